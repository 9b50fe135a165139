// Formulation A, the workgroup-per-QP solver ismpc_a_tick_kernel: one 256-thread workgroup per QP, an explicit S^-1 = (N' H^-1 N)^-1 of
// working-set size, rank-1 border / Schur updates, two refinement passes.  A handle runs it when F is outside the wave kernels' 3..6 or
// under ISMPC_A_KERNEL=block (A/B); tests/test_gpu_formulation_a.py::test_workgroup_kernel_against_oracle is its pin.
#pragma once
#include <hip/hip_runtime.h>
#include "ismpc_a_dev.hpp"
#include "ismpc_wave_prims.hpp"

namespace {

using ismpc_a::DevA;
constexpr int T = ismpc_a::WG;         // threads per workgroup; requires C + F <= 256
constexpr int MAXF = ismpc_a::MAXF;
constexpr int QCAP = 264;              // capacity of the working set (>= C + F + 1)

// ---- wave / block primitives ------------------------------------------------------------------
using ismpc_wave::wave_scan_up;       // inclusive prefix sum over the 64 lanes

struct Shared {
    double u[T], zu[T], imp[T], zlo[T], zhi[T], w1[T], w2[T], a[T], PA[T + 1];
    int k1[T];
    double f[MAXF + 1], zf[MAXF + 1], pref[MAXF + 1], klo[MAXF + 1], khi[MAXF + 1];
    int act_row[QCAP]; double act_sgn[QCAP], mu[QCAP], r[QCAP], dp[QCAP];
    int state[T + MAXF + 1];            // per row (1..C+F): 0 free, +1 lower active, -1 upper active
    double red[T]; int redi[T];
    double wsum[8];
    double zfpart[4][MAXF + 1];
    // scalars
    double b, sviol, sg, gamma, npn, t, t1, t2, mu_p, rowval;
    int q, row, drop, flag, iters, status;
};

// inclusive prefix sum over the workgroup (thread order); every thread calls
__device__ __forceinline__ double block_scan_incl(Shared& s, double v, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    const double p = wave_scan_up(v);
    if (lane == 63) s.wsum[wave] = p;
    __syncthreads();
    double add = 0.0;
    for (int wv = 0; wv < wave; ++wv) add += s.wsum[wv];
    __syncthreads();
    return p + add;
}
// inclusive prefix sum plus the workgroup total
__device__ __forceinline__ double block_scan_incl_tot(Shared& s, double v, int tid, double& tot)
{
    const int lane = tid & 63, wave = tid >> 6;
    const double p = wave_scan_up(v);
    if (lane == 63) s.wsum[wave] = p;
    __syncthreads();
    double add = 0.0;
    for (int wv = 0; wv < wave; ++wv) add += s.wsum[wv];
    tot = ((s.wsum[0] + s.wsum[1]) + s.wsum[2]) + s.wsum[3];
    __syncthreads();
    return p + add;
}
// sum over the workgroup, same value (bitwise) in every thread
__device__ __forceinline__ double block_sum(Shared& s, double v, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    const double p = wave_scan_up(v);
    if (lane == 63) s.wsum[wave] = p;
    __syncthreads();
    const double tot = ((s.wsum[0] + s.wsum[1]) + s.wsum[2]) + s.wsum[3];
    __syncthreads();
    return tot;
}
// minimum of v with its index (ties: smallest index), broadcast to all threads; v = +inf means "no candidate"
__device__ __forceinline__ void block_argmin(Shared& s, double v, int idx, int tid, double& vmin, int& imin)
{
    s.red[tid] = v; s.redi[tid] = idx;
    __syncthreads();
    if (tid < 16) {
        double bv = s.red[tid * 16]; int bi = s.redi[tid * 16];
        for (int k = 1; k < 16; ++k) {
            const double cv = s.red[tid * 16 + k]; const int ci = s.redi[tid * 16 + k];
            if (cv < bv || (cv == bv && ci < bi)) { bv = cv; bi = ci; }
        }
        s.red[tid * 16] = bv; s.redi[tid * 16] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        double bv = s.red[0]; int bi = s.redi[0];
        for (int k = 1; k < 16; ++k) {
            const double cv = s.red[k * 16]; const int ci = s.redi[k * 16];
            if (cv < bv || (cv == bv && ci < bi)) { bv = cv; bi = ci; }
        }
        s.red[0] = bv; s.redi[0] = bi;
    }
    __syncthreads();
    vmin = s.red[0]; imin = s.redi[0];
    __syncthreads();
}

// ---- closed-form H^-1 inner products of constraint rows (row 0 = stability, 1..C = ZMP, C+1..C+F = kinematic)
__device__ __forceinline__ double mdot(const Shared& s, int i, int k)   // M_i . M_k over the footstep columns 1..F
{
    const int a1 = s.k1[i - 1], b1 = s.k1[k - 1];
    const double aw1 = s.w1[i - 1], aw2 = s.w2[i - 1], bw1 = s.w1[k - 1], bw2 = s.w2[k - 1];
    double acc = 0.0;
    // entries: (a1 -> aw1), (a1+1 -> aw2) ; column 0 is the current footstep (not a variable)
    if (a1 >= 1) { if (a1 == b1) acc += aw1 * bw1; else if (a1 == b1 + 1) acc += aw1 * bw2; }
    { const int c = a1 + 1; if (c == b1 && b1 >= 1) acc += aw2 * bw1; else if (c == b1 + 1) acc += aw2 * bw2; }
    return acc;
}
__device__ __forceinline__ double mcol(const Shared& s, int i, int r)   // M_i[r], r in 1..F (0 outside)
{
    if (r < 1) return 0.0;
    const int a1 = s.k1[i - 1];
    if (r == a1) return s.w1[i - 1];
    if (r == a1 + 1) return s.w2[i - 1];
    return 0.0;
}
__device__ __forceinline__ double ip_rows(const Shared& s, const DevA& c, int r1, int r2)
{
    if (r1 > r2) { const int t_ = r1; r1 = r2; r2 = t_; }
    const int C = c.C;
    if (r1 == 0) {
        if (r2 == 0) return c.aa;
        if (r2 <= C) return c.dt * s.PA[r2];
        return 0.0;
    }
    if (r2 <= C) return c.dt * c.dt * (double)r1 + mdot(s, r1, r2) / c.Qf;       // min(r1, r2) = r1
    if (r1 <= C) { const int r = r2 - C; return (-mcol(s, r1, r) + mcol(s, r1, r - 1)) / c.Qf; }
    const int ra = r1 - C, rb = r2 - C;
    if (ra == rb) return (1.0 + (ra >= 2 ? 1.0 : 0.0)) / c.Qf;
    return (rb - ra == 1) ? -1.0 / c.Qf : 0.0;
}

// x += H^-1 N coef : adds  sum_j coef_j * (row_j)  scaled by H^-1 to (u, f).  coef[j] for j < q in s.dp (signed,
// already multiplied by the row's sign); optional extra row `xrow` with coefficient xc.  Result in s.zu / s.zf.
__device__ __forceinline__ void build_direction(Shared& s, const DevA& c, int tid, int q, int xrow, double xc)
{
    const int C = c.C, F = c.F;
    if (tid < C) s.imp[tid] = 0.0;
    __syncthreads();
    // ZMP rows: dt on u[0..i-1]  ->  impulse at i-1, suffix-summed below (a row is active at most once)
    double fpart[MAXF + 1];
#pragma unroll
    for (int k = 0; k <= MAXF; ++k) fpart[k] = 0.0;
    double ce = 0.0;
    for (int j = tid; j <= q; j += T) {
        int row; double cf;
        if (j < q) { row = s.act_row[j]; cf = s.dp[j]; } else { row = xrow; cf = xc; }
        if (row < 0 || cf == 0.0) continue;
        if (row == 0) ce += cf;
        else if (row <= C) {
            s.imp[row - 1] += cf * c.dt;
            const int a1 = s.k1[row - 1];
            if (a1 >= 1) fpart[a1] -= cf * s.w1[row - 1];
            if (a1 + 1 <= F) fpart[a1 + 1] -= cf * s.w2[row - 1];
        } else {
            const int r = row - C;
            fpart[r] += cf;
            if (r >= 2) fpart[r - 1] -= cf;
        }
    }
    // note: two different active ZMP rows never share an index, and the extra row is not active: no write race
    // stability coefficient and footstep parts: one wave scan each, ONE barrier, fixed-order combine (bit reproducible)
    {
        const int lane = tid & 63, wave = tid >> 6;
        const double pe = wave_scan_up(ce);
        if (lane == 63) s.zfpart[wave][0] = pe;
        for (int k = 1; k <= F; ++k) {
            const double pk = wave_scan_up(fpart[k]);
            if (lane == 63) s.zfpart[wave][k] = pk;
        }
    }
    __syncthreads();
    const double cetot = ((s.zfpart[0][0] + s.zfpart[1][0]) + s.zfpart[2][0]) + s.zfpart[3][0];
    if (tid >= 1 && tid <= F) s.zf[tid] = (((s.zfpart[0][tid] + s.zfpart[1][tid]) + s.zfpart[2][tid]) + s.zfpart[3][tid]) / c.Qf;
    // suffix sum of the impulses = total - exclusive prefix
    const double v = (tid < C) ? s.imp[tid] : 0.0;
    double tot;
    const double incl = block_scan_incl_tot(s, v, tid, tot);
    if (tid < C) s.zu[tid] = (tot - (incl - v)) + cetot * s.a[tid];
    __syncthreads();
}

// value of constraint rows for the current x: thread tid < C gets zeta_{tid+1}, threads C..C+F-1 get kin_{tid-C+1}
__device__ __forceinline__ double row_value(Shared& s, const DevA& c, int tid)
{
    const int C = c.C, F = c.F;
    const double cum = block_scan_incl(s, (tid < C) ? s.u[tid] : 0.0, tid);
    if (tid < C) {
        const int a1 = s.k1[tid];
        double mf = 0.0;
        if (a1 >= 1) mf += s.w1[tid] * s.f[a1];
        if (a1 + 1 <= F) mf += s.w2[tid] * s.f[a1 + 1];
        return c.dt * cum - mf;
    }
    if (tid < C + F) { const int r = tid - C + 1; return s.f[r] - (r >= 2 ? s.f[r - 1] : 0.0); }
    return 0.0;
}

// HZ: the tick also stores the whole decision of every QP into `dec` (ismpc_a_tick_batch_horizon_device; the layout is stated in
// include/ismpc_a.h).  <false> is the tick as it always was: `dec` is never read and no store exists.
template <bool HZ>
__global__ __launch_bounds__(T)
void ismpc_a_tick_kernel(const DevA c, const ismpc_a_state* __restrict__ state_in, ismpc_a_state* __restrict__ state,
                         const double* __restrict__ push, ismpc_a_out* __restrict__ out, int batch, double* __restrict__ dec)
{
    __shared__ Shared s;
    extern __shared__ double sinv_lds[];            // ldq x ldq when the launch asked for it (c.sinv_in_lds)
    const int tid = threadIdx.x;
    const int C = c.C, F = c.F, P = c.P;
    double* Sinv = c.sinv_in_lds ? sinv_lds : c.scratch + (size_t)blockIdx.x * c.ldq * c.ldq;
    const int ldq = c.ldq;

    for (int work = blockIdx.x; work < 2 * batch; work += gridDim.x) {
        const int inst = work >> 1, axis = work & 1;
        // the two axes of an instance are separate work items: both read the PREVIOUS state (state_in, a copy
        // made by the host entry point) and each writes only its own fields of `state`
        const ismpc_a_state st = state_in[inst];
        const double pos = axis == 0 ? st.x : st.y;
        const double vel = (axis == 0 ? st.xd : st.yd) + (push ? push[inst * 2 + axis] : 0.0);
        const double zmp = axis == 0 ? st.xz : st.yz;
        const double cur = axis == 0 ? st.cur_x : st.cur_y;
        const double off = axis == 0 ? st.off_x : st.off_y;
        const int j = st.j, fc = st.fc;
        const double* fs = axis == 0 ? c.fsx : c.fsy;
        const double* cl = st.rebuilt ? (axis == 0 ? c.clx1 : c.cly1) : (axis == 0 ? c.clx0 : c.cly0);
        const double cloff = st.rebuilt ? off : 0.0;
        int status = 0;
        // ---- validity of indices: fs_plan(fc+1 .. fc+F), cl(j+C+1 .. j+P), j inside step fc
        if (fc < 1 || fc + F > c.n_gait || j < 1 || j + P > c.ncl || j < c.step * (fc - 1) || j > c.step * fc - 1)
            status |= ISMPC_A_ST_BAD_INDEX;

        // ---- mapping (quad_walk_no_plots.m:153-171), bounds (:173-181), stability data
        if (tid < C) {
            const int i = tid + 1;
            int pf = (j + i) / c.step - fc + 1; if (pf < 0) pf = 0;
            const int rem = c.step * (fc + pf) - (j + i);
            double w1, w2;
            if (rem > c.ds) { w1 = 1.0; w2 = 0.0; } else { w1 = (double)rem / c.ds; w2 = 1.0 - (double)rem / c.ds; }
            s.k1[tid] = pf; s.w1[tid] = w1; s.w2[tid] = w2;
            const double m1 = (pf == 0) ? w1 : 0.0;
            s.zhi[tid] = 1.0 * (-zmp + c.w / 2) + m1 * cur;
            s.zlo[tid] = -(-1.0 * (-zmp - c.w / 2) - m1 * cur);
            s.a[tid] = c.a[tid]; s.u[tid] = 0.0;
            s.red[tid] = (pf > F || (w2 != 0.0 && pf + 1 > F) || (rem <= c.ds && pf + 1 > F)) ? 1.0 : 0.0;
        } else s.red[tid] = 0.0;
        for (int k = tid; k <= C; k += T) s.PA[k] = c.PA[k];
        for (int k = tid; k < C + F + 1; k += T) s.state[k] = 0;
        __syncthreads();
        const double ovf = block_sum(s, s.red[tid], tid);
        if (ovf > 0.0) status |= ISMPC_A_ST_OVERFLOW;
        // anticipative tail (:227-231), xfs_store(fsCounter) == current footstep
        double tl = 0.0;
        if (!(status & ISMPC_A_ST_BAD_INDEX))
            for (int i = C + 1 + tid; i <= P; i += T) tl += c.wtail[i - (C + 1)] * ((cl[j + i - 1] + cloff) - cur);
        double tail = block_sum(s, tl, tid);
        if (!(status & ISMPC_A_ST_BAD_INDEX)) tail += c.wP * ((cl[P - 1] + cloff) - cur);
        if (tid == 0) {
            s.b = pos + vel / c.eta - zmp - tail;
            for (int r = 1; r <= F; ++r) {
                double bup = axis == 0 ? c.disp_forw : (c.disp_L / 2 + c.disp_L / 2);
                if (fc == 1 && r == 1) bup = axis == 0 ? c.disp_forw_dummy : (c.disp_L / 2 + c.disp_L / 2);
                double blo = bup;
                if (r == 1) { bup = bup + cur; blo = blo - cur; }
                s.khi[r] = bup; s.klo[r] = -blo;
                const double pr = (status & ISMPC_A_ST_BAD_INDEX) ? 0.0 : fs[fc + r - 1] + off;
                s.pref[r] = pr; s.f[r] = pr;                       // unconstrained minimiser: u = 0, f = p
            }
            s.q = 0; s.iters = 0; s.status = status;
        }
        __syncthreads();

        int q = 0, iters = 0;
        if (status == 0) {
            // ---- equality first: n = (a, 0); from x = (0, p): t = b / a'a
            {
                const double t0 = s.b / c.aa;
                if (tid < C) s.u[tid] = t0 * s.a[tid];
                if (tid == 0) { s.act_row[0] = 0; s.act_sgn[0] = 1.0; s.mu[0] = t0; Sinv[0] = 1.0 / c.aa; }
                q = 1;
                __syncthreads();
            }
            bool resumed = false;
            for (;;) {
                // ======== outer: most violated inactive row (normalised by its H^-1 norm) ========
                const double v = row_value(s, c, tid);
                double cand = INFINITY; int cidx = 0;
                if (tid < C + F) {
                    const int row = tid + 1;
                    if (s.state[row] == 0) {
                        const double lo = tid < C ? s.zlo[tid] : s.klo[tid - C + 1];
                        const double hi = tid < C ? s.zhi[tid] : s.khi[tid - C + 1];
                        const double vl = v - lo, vh = hi - v;
                        const double tol = 1e-11 * (fabs(v) + fmax(fabs(lo), fabs(hi))) + 1e-13;
                        const double nrm = sqrt(ip_rows(s, c, row, row));
                        if (vl < -tol) { cand = vl / nrm; cidx = 2 * row; }
                        if (vh < -tol && vh / nrm < cand) { cand = vh / nrm; cidx = 2 * row + 1; }
                    }
                }
                double vmin; int imin;
                block_argmin(s, cand, cidx, tid, vmin, imin);
                if (!(vmin < 0.0)) {
                    // ---- converged on this working set: two refinement passes (N'x = bounds exactly), then re-check
                    if (resumed) break;
                    for (int pass = 0; pass < 2; ++pass) {
                        const double vv = row_value(s, c, tid);
                        if (tid < C + F && s.state[tid + 1] != 0) s.red[tid] = vv;
                        __syncthreads();
                        // residual per active row (signed), then dm = S^-1 res
                        if (tid < q) {
                            const int row = s.act_row[tid];
                            double res;
                            if (row == 0) {
                                res = 0.0;      // filled below by the block (needs a'u)
                            } else {
                                const double sgn = s.act_sgn[tid];
                                const double bound = row <= C ? (sgn > 0 ? s.zlo[row - 1] : s.zhi[row - 1])
                                                              : (sgn > 0 ? s.klo[row - C] : s.khi[row - C]);
                                res = sgn * (bound - s.red[row - 1]);
                            }
                            s.r[tid] = res;
                        }
                        const double au = block_sum(s, (tid < C) ? s.a[tid] * s.u[tid] : 0.0, tid);
                        if (tid == 0) s.r[0] = s.b - au;
                        __syncthreads();
                        if (tid < q) {
                            double acc = 0.0;
#pragma unroll 8
                            for (int k = 0; k < q; ++k) acc += Sinv[(size_t)k * ldq + tid] * s.r[k];
                            s.dp[tid] = acc * s.act_sgn[tid];
                        }
                        __syncthreads();
                        build_direction(s, c, tid, q, -1, 0.0);
                        if (tid < C) s.u[tid] += s.zu[tid];
                        if (tid >= 1 && tid <= F) s.f[tid] += s.zf[tid];
                        __syncthreads();
                    }
                    resumed = true;
                    continue;                                   // one more feasibility sweep
                }
                resumed = false;
                const int row = imin >> 1;
                const double sg = (imin & 1) ? -1.0 : 1.0;
                double sviol;
                {
                    const int rt = row - 1;                      // thread that holds this row's value
                    if (tid == rt) {
                        const double lo = rt < C ? s.zlo[rt] : s.klo[rt - C + 1];
                        const double hi = rt < C ? s.zhi[rt] : s.khi[rt - C + 1];
                        s.sviol = sg > 0 ? v - lo : hi - v;
                    }
                    __syncthreads();
                    sviol = s.sviol;
                }
                double mu_p = 0.0;
                const double npn = ip_rows(s, c, row, row);
                // ======== inner: steps until the row is added (Goldfarb-Idnani step logic) ========
                for (;;) {
                    if (++iters > c.max_iter) { status |= ISMPC_A_ST_ITER_LIMIT; break; }
                    // d = N' H^-1 n+
                    if (tid < q) s.dp[tid] = sg * s.act_sgn[tid] * ip_rows(s, c, row, s.act_row[tid]);
                    __syncthreads();
                    // r = S^-1 d
                    double racc = 0.0;
                    if (tid < q) {
#pragma unroll 8
                        for (int k = 0; k < q; ++k) racc += Sinv[(size_t)k * ldq + tid] * s.dp[k];
                        s.r[tid] = racc;
                    }
                    const double dr = block_sum(s, (tid < q) ? s.dp[tid] * racc : 0.0, tid);
                    const double gamma = npn - dr;
                    // dual step length: min over active inequalities with r > 0 of mu / r
                    double tc = INFINITY;
                    if (tid >= 1 && tid < q && racc > 0.0) tc = s.mu[tid] / racc;
                    double t1; int l;
                    block_argmin(s, tc, tid, tid, t1, l);
                    const double t2 = (gamma > 1e-12 * npn) ? -sviol / gamma : INFINITY;
                    const double t = fmin(t1, t2);
                    if (!(t < INFINITY)) { status |= (axis == 0 ? ISMPC_A_ST_X_INFEASIBLE : ISMPC_A_ST_Y_INFEASIBLE); break; }
                    if (t2 < INFINITY) {
                        // z = H^-1 (n+ - N r): coefficients -r_j sign_j on the active rows, +sg on the new one
                        if (tid < q) s.dp[tid] = -racc * s.act_sgn[tid];
                        __syncthreads();
                        build_direction(s, c, tid, q, row, sg);
                        if (tid < C) s.u[tid] += t * s.zu[tid];
                        if (tid >= 1 && tid <= F) s.f[tid] += t * s.zf[tid];
                    }
                    if (tid < q) s.mu[tid] -= t * racc;
                    mu_p += t;
                    __syncthreads();
                    if (t2 < INFINITY && t == t2) {
                        // ---- full step: border update of S^-1, append the row
                        const double ig = 1.0 / gamma;
                        if (tid < q) {
                            const double rj = s.r[tid];
#pragma unroll 8
                            for (int k = 0; k < q; ++k) Sinv[(size_t)k * ldq + tid] += s.r[k] * rj * ig;
                            Sinv[(size_t)q * ldq + tid] = -rj * ig;
                            Sinv[(size_t)tid * ldq + q] = -rj * ig;
                        }
                        if (tid == 0) {
                            Sinv[(size_t)q * ldq + q] = ig;
                            s.act_row[q] = row; s.act_sgn[q] = sg; s.mu[q] = mu_p; s.state[row] = sg > 0 ? 1 : -1;
                        }
                        ++q;
                        __syncthreads();
                        break;
                    }
                    // ---- partial step: drop working-set entry l (Schur update), keep going with the same row
                    {
                        const double piv = Sinv[(size_t)l * ldq + l];
                        __syncthreads();
                        if (tid < q) s.r[tid] = Sinv[(size_t)l * ldq + tid];      // column l (symmetric)
                        __syncthreads();
                        if (tid < q && tid != l) {
                            const double cj = s.r[tid] / piv;
#pragma unroll 8
                            for (int k = 0; k < q; ++k) if (k != l) Sinv[(size_t)k * ldq + tid] -= s.r[k] * cj;
                        }
                        __syncthreads();
                        // move the last entry into slot l
                        const int last = q - 1;
                        if (l != last) {
                            if (tid < q && tid != l) {
                                const double vlast = Sinv[(size_t)last * ldq + tid];
                                Sinv[(size_t)l * ldq + tid] = vlast;
                                Sinv[(size_t)tid * ldq + l] = vlast;
                            }
                            __syncthreads();
                            if (tid == 0) Sinv[(size_t)l * ldq + l] = Sinv[(size_t)last * ldq + last];
                        }
                        if (tid == 0) {
                            s.state[s.act_row[l]] = 0;
                            if (l != last) { s.act_row[l] = s.act_row[last]; s.act_sgn[l] = s.act_sgn[last]; s.mu[l] = s.mu[last]; }
                        }
                        --q;
                        __syncthreads();
                    }
                    // violation of the row at the new point
                    {
                        const double vv = row_value(s, c, tid);
                        const int rt = row - 1;
                        if (tid == rt) {
                            const double lo = rt < C ? s.zlo[rt] : s.klo[rt - C + 1];
                            const double hi = rt < C ? s.zhi[rt] : s.khi[rt - C + 1];
                            s.sviol = sg > 0 ? vv - lo : hi - vv;
                        }
                        __syncthreads();
                        sviol = s.sviol;
                    }
                }
                if (status != 0) break;
            }
        }

        // ---- LIP update (:297-322), footstep bookkeeping (:522-556), outputs
        __syncthreads();
        if constexpr (HZ) {
            // u[0 .. C-1] and the absolute footsteps f[1 .. F] as they stand in LDS: slot 0 is u0 and slot C is f0 below, to the bit; an
            // instance the tick leaves alone has u = 0 and every footstep = f0 = cur
            const bool left = (status & (ISMPC_A_ST_BAD_INDEX | ISMPC_A_ST_OVERFLOW)) != 0;
            double* dq = dec + (size_t)work * (size_t)(C + F);
            if (tid < C) dq[tid] = left ? 0.0 : s.u[tid];
            if (tid < F) dq[C + tid] = left ? cur : s.f[tid + 1];
        }
        if (tid == 0) {
            const double u0 = (status & (ISMPC_A_ST_BAD_INDEX | ISMPC_A_ST_OVERFLOW)) ? 0.0 : s.u[0];
            const double f0 = (status & (ISMPC_A_ST_BAD_INDEX | ISMPC_A_ST_OVERFLOW)) ? cur : s.f[1];
            const double p0 = pos, v0 = vel, z0 = zmp;
            const double np_ = (c.Au[0] * p0 + c.Au[1] * v0 + c.Au[2] * z0) + c.Bu[0] * u0;
            const double nv_ = (c.Au[3] * p0 + c.Au[4] * v0 + c.Au[5] * z0) + c.Bu[1] * u0;
            const double nz_ = (c.Au[6] * p0 + c.Au[7] * v0 + c.Au[8] * z0) + c.Bu[2] * u0;
            ismpc_a_state* so = state + inst;
            const bool ok = (status & (ISMPC_A_ST_BAD_INDEX | ISMPC_A_ST_OVERFLOW)) == 0;
            const bool stepped = ok && (j + 1 >= c.step * fc);
            if (ok) {
                if (axis == 0) { so->x = np_; so->xd = nv_; so->xz = nz_; } else { so->y = np_; so->yd = nv_; so->yz = nz_; }
                if (stepped) {
                    const double noff = f0 - fs[fc];                  // predicted - fs_plan(fc+1)  (base plan)
                    if (axis == 0) { so->cur_x = f0; so->off_x = noff; } else { so->cur_y = f0; so->off_y = noff; }
                }
                if (axis == 0) { so->j = j + 1; if (stepped) { so->fc = fc + 1; so->rebuilt = 1; } }
            }
            if (out) {
                ismpc_a_out* o = out + inst;
                o->com_before[axis] = pos; o->vel_after[axis] = ok ? nv_ : vel; o->u0[axis] = u0; o->f0[axis] = f0;
                if (axis == 0) { o->iters_x = iters; atomicOr(&o->status, status); atomicOr(&o->active, q & 0xffff); }
                else { o->iters_y = iters; atomicOr(&o->status, status); atomicOr(&o->active, (q & 0xffff) << 16); }
            }
        }
        __syncthreads();
    }
}

}  // namespace
