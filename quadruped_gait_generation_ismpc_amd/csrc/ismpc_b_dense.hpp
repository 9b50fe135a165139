// Formulation B, part 2 of 4 of the translation unit ismpc_hip.hip: the dense per-tick solve (ISMPC_PATH=dense; kept for A/B and
// as the per-tick MFMA formulation).  One launch = one MPCSolver::solve (reference AMR_code_DART/MPCSolver.cpp:204-430)
// for every instance of a batch.  A 256-thread workgroup (4 wavefronts) owns
// 16 instances -- the row tile of v_mfma_f64_16x16x4_f64:
//
//   phase A  (wave per instance, lanes = horizon samples)
//            f_z of MPCSolver.cpp:259, with S_bar_z' and S_bar_z_v' applied as
//            suffix sums (they are Toeplitz-triangular, :144-154) -> LDS F[16][NP]
//   phase B  (MFMA)  U = -F * Hinv : the only dense contraction of the tick.
//            Hinv = (q_p S'S + q_v Sv'Sv + q_u I)^-1 is constant (the reference
//            re-forms the Hessian every tick at :258 although it never changes)
//            and shared by the whole batch; B operand streamed from L2.
//   phase C  (wave per instance)
//            - u_i = 0 equalities of :223-243 by a rank-<=F correction
//              (one table column per equality row, chosen by mpcIter)
//            - 0 <= S_bar_z u <= 1e4 check (:158-160), z integration (:274-278)
//            - lambda_j (:296-309), A_j/B_j (:353-361)
//            - phi_state / phi_input (:362-371) as ONE suffix scan of 2x2
//              matrices instead of the reference's O(N^2) cosh/sinh loop
//            - both horizontal QPs (:395-396: H = I, one equality row, a box)
//              solved exactly as continuous quadratic knapsacks
//            - integration (:406-422), 80-byte output record.
#pragma once
#include "ismpc_b_common.hpp"

namespace {

constexpr int TI = 16;          // instances per workgroup = MFMA M tile

typedef double d4 __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ M2 dpp_m2_ident(const M2& y)     // out-of-range source lane -> identity
{
    M2 t;
    t.a = dppv<CTRL, 0xf, false>(1.0, y.a); t.b = dppv<CTRL, 0xf, false>(0.0, y.b);
    t.c = dppv<CTRL, 0xf, false>(0.0, y.c); t.d = dppv<CTRL, 0xf, false>(1.0, y.d);
    return t;
}
// X_lane = Y_63 Y_62 ... Y_{lane+1} (identity for lane 63); total = Y_63 ... Y_0
__device__ __forceinline__ M2 wave_suffix_product_excl(M2 y, int lane, M2& total)
{
    y = mul(dpp_m2_ident<0x101>(y), y);       // row_shl:1  (lane L reads lane L+1 of its row)
    y = mul(dpp_m2_ident<0x102>(y), y);
    y = mul(dpp_m2_ident<0x104>(y), y);
    y = mul(dpp_m2_ident<0x108>(y), y);
    // first lane of each 16-lane row now holds that row's product; fold the rows above in
    const M2 p1 = readlane_m2<16>(y), p2 = readlane_m2<32>(y), p3 = readlane_m2<48>(y);
    const M2 m1 = mul(p3, p2), m0 = mul(m1, p1);
    const int row = lane >> 4;
    M2 pre = (M2){1.0, 0.0, 0.0, 1.0};
    if (row == 2) pre = p3; else if (row == 1) pre = m1; else if (row == 0) pre = m0;
    y = mul(pre, y);
    total = readlane_m2<0>(y);
    return dpp_m2_ident<0x130>(y);            // wave_shl:1 -> exclusive
}

// R = horizon samples per lane (N <= 64 R); WAVES = wavefronts per workgroup (16 instances per
// workgroup either way, each wavefront walks TI / WAVES of them through phases A and C).
template <int R, int WAVES>
__global__ __launch_bounds__(64 * WAVES)
void ismpc_tick_dense(const DevConst c, const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                       ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj, int batch, int rollout_frame)
{
    constexpr int IPW = TI / WAVES;
    extern __shared__ double smem[];                  // [TI][NPs]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int inst0 = blockIdx.x * TI;
    const int N = c.N, NP = c.NP, NPs = c.NPs;
    const double dt = c.dt;
    const ismpc_tick_in* in = (rollout_frame >= 0) ? state_rw : in_ro;

    // ---------------- phase A: f_z, MPCSolver.cpp:259 ----------------
    // lanes hold the horizon REVERSED here (lane L <-> samples (63-L) R ..): S_bar_z' and S_bar_z_v'
    // are sums over LATER samples, which this way are prefix sums over lanes (DPP row_shr / row_bcast).
    for (int q = 0; q < IPW; ++q) {
        const int li = wave * IPW + q;
        const int gi = inst0 + li;
        const int nb = (63 - lane) * R;
        double f[R];
#pragma unroll
        for (int r = 0; r < R; ++r) f[r] = 0.0;
        if (gi < batch) {
            const Walk w = load_walk(c, in + gi, rollout_frame);
            int idx;
            if (gate_tick(c, w, idx) == 0) {
                const double z = in[gi].com_pos[2], zd = in[gi].com_vel[2];
                double rp[R], rv[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int n = nb + r;
                    if (n < N) {
                        const double k = (double)n;
                        // T_bar_z(k,:) s + T_bar_g_z(k) - h_des - mid_z ; T_bar_z_v(k,:) s + T_bar_g_z_v(k)
                        rp[r] = (z + (k + 1.0) * dt * zd) - c.g * dt * dt * (0.5 * k * (k + 1.0)) - c.h_des - c.midz[idx + n];
                        rv[r] = zd - c.g * dt * k;
                    } else { rp[r] = 0.0; rv[r] = 0.0; }
                }
                // T_j = sum_{k>=j} rp_k ;  V_i = sum_{j>i} T_j = sum_{k>i} (k-i) rp_k ;  TV_i = sum_{k>i} rv_k
                double tp[R], lp = 0.0, lv = 0.0, tv[R];
#pragma unroll
                for (int r = R - 1; r >= 0; --r) { tv[r] = lv; lv += rv[r]; lp += rp[r]; tp[r] = lp; }
                const double up = wave_prefix_excl(lp);
                const double uv = wave_prefix_excl(lv);
                double vt[R], lt = 0.0;
#pragma unroll
                for (int r = R - 1; r >= 0; --r) { tp[r] += up; vt[r] = lt; lt += tp[r]; }
                const double ut = wave_prefix_excl(lt);
                const double cs = dt * dt / c.mass, cv = dt / c.mass;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int n = nb + r;
                    if (n < N) f[r] = c.q_p * cs * (vt[r] + ut) + c.q_v * cv * (tv[r] + uv) - c.q_u * c.mass * c.g;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) { const int n = nb + r; if (n < NP) smem[li * NPs + n] = f[r]; }
    }
    __syncthreads();

    // ---------------- phase B: U = -F Hinv on the matrix cores ----------------
    {
        constexpr int MAXT = (16 + WAVES - 1) / WAVES;   // NP <= 256 -> at most 16 column tiles
        const int ntiles = NP >> 4;
        d4 acc[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
        const int arow = lane & 15, kq = lane >> 4;
        if (wave < ntiles) {
            for (int kk = 0; kk < NP; kk += 4) {
                const double a = smem[arow * NPs + kk + kq];                   // A[i = lane&15][k = lane>>4]
                const double* brow = c.Hinv + (size_t)(kk + kq) * NP + arow;   // B[k = lane>>4][j = lane&15]
#pragma unroll
                for (int t = 0; t < MAXT; ++t) {
                    const int tile = wave + t * WAVES;
                    if (tile < ntiles) {
                        const double b = brow[tile * 16];
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                               // every wave is done reading F
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int tile = wave + t * WAVES;
            if (tile < ntiles) {
#pragma unroll
                for (int v = 0; v < 4; ++v)            // D: col = lane&15, row = (lane>>4) + 4*v
                    smem[(kq + 4 * v) * NPs + tile * 16 + arow] = -acc[t][v];
            }
        }
    }
    __syncthreads();

    // ---------------- phase C: everything after the vertical solve ----------------
    for (int q = 0; q < IPW; ++q) {
        const int li = wave * IPW + q;
        const int gi = inst0 + li;
        if (gi >= batch) continue;
        const ismpc_tick_in* rec = in + gi;
        const Walk w = load_walk(c, rec, rollout_frame);
        const double x0 = rec->com_pos[0], y0 = rec->com_pos[1], z0 = rec->com_pos[2];
        const double xd0 = rec->com_vel[0], yd0 = rec->com_vel[1], zd0 = rec->com_vel[2];
        int idx;
        int status = gate_tick(c, w, idx);
        double o_x = x0, o_y = y0, o_z = z0, o_xd = xd0, o_yd = yd0, o_zd = zd0;
        double uz0 = 0.0, ux0 = 0.0, uy0 = 0.0;
        int itx = 0, ity = 0;
        double u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = 0.0;
        double tau[2] = {0.0, 0.0}, sgx = 1.0, sgy = 1.0, hbox = 0.0;
        double a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = 0.0;
        bool stage3 = false;

        if (status == 0) {
            // ---- stage 1 tail: equality correction (MPCSolver.cpp:223-243, is_running :262-263)
#pragma unroll
            for (int r = 0; r < R; ++r) { const int n = lane * R + r; u[r] = (n < N) ? smem[li * NPs + n] : 0.0; }
            if (w.fc > 1 && w.mpc < c.npat) {
                const int elo = c.e_lo[w.mpc], ne = c.ne[w.mpc];
                const double* Wp = c.W + (size_t)w.mpc * c.Fmax * NP;
                for (int e = 0; e < ne; ++e) {
                    const double ue = smem[li * NPs + elo + e];
#pragma unroll
                    for (int r = 0; r < R; ++r) { const int n = lane * R + r; if (n < N) u[r] -= Wp[(size_t)e * NP + n] * ue; }
                }
#pragma unroll
                for (int r = 0; r < R; ++r) { const int n = lane * R + r; if (n >= elo && n < elo + ne) u[r] = 0.0; }
            }
            // ---- S_bar_z u = (dt^2/m) * exclusive prefix of inclusive prefix of u
            double ci[R], lc = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) { lc += u[r]; ci[r] = lc; }
            const double pc = wave_prefix_excl(lc);
            double di[R], ld_ = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) { ci[r] += pc; di[r] = ld_; ld_ += ci[r]; }
            const double pd = wave_prefix_excl(ld_);
            const double cs = dt * dt / c.mass;
            bool viol = false;
            double lam[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = lane * R + r;
                const double k = (double)n;
                const double su = cs * (di[r] + pd);
                if (n < N && (su < c.z_lo - 1e-11 * fmax(1.0, fabs(c.z_lo)) || su > c.z_hi + 1e-11 * fmax(1.0, fabs(c.z_hi)))) viol = true;   // beyond rounding
                const double zpos = su + (z0 + (k + 1.0) * dt * zd0) - c.g * dt * dt * (0.5 * k * (k + 1.0));
                const double zacc = (1.0 / c.mass) * u[r] - c.g;
                lam[r] = (c.g + zacc) / zpos;                               // MPCSolver.cpp:306
            }
            if (__builtin_amdgcn_ballot_w64(viol) != 0) status |= ISMPC_ST_Z_INEQ_ACTIVE;
            uz0 = bcast0(u[0]);
            // ---- z integration, MPCSolver.cpp:274-278
            o_z = z0 + dt * zd0;
            o_zd = zd0 + (dt / c.mass) * uz0 - dt * c.g;
            if (isnan(o_z)) { o_z = c.h_des; status |= ISMPC_ST_Z_NAN; }
            if (isnan(o_zd)) { o_zd = 0.0; status |= ISMPC_ST_Z_NAN; }

            // ---- A_j, B_j per sample, MPCSolver.cpp:353-361, in the form
            //   A = [1 + wQ, dt P; lambda dt P, 1 + wQ],  B = [-wQ, -lambda dt P],  w = lambda dt^2,
            //   P = sinh(x)/x, Q = (cosh(x)-1)/x^2, x = sqrt(lambda) dt: no sqrt, no division, and
            //   lambda < gate (A = [1 dt; 0 1], B = 0) is simply lambda := 0.
            M2 A[R]; double B0[R], B1[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = lane * R + r;
                const double le = (lam[r] < c.gate) ? 0.0 : lam[r];
                const double dtn = (n < N) ? dt : 0.0;
                const double wv = le * dtn * dtn;
                double P, Q;
                sinhc_coshc(wv, P, Q);
                const double ch1 = wv * Q, s1 = dtn * P, s2 = le * s1;
                A[r] = (M2){1.0 + ch1, s1, s2, 1.0 + ch1};
                B0[r] = -ch1; B1[r] = -s2;
            }
            const double lam0 = bcast0(lam[0]);
            const M2 A0 = readlane_m2<0>(A[0]);
            const double B00 = bcast0(B0[0]), B10 = bcast0(B1[0]);

            if (lam0 > c.gate) {                                           // MPCSolver.cpp:322
                stage3 = true;
                // ---- suffix products: X_lane = A_{N-1} ... A_{first sample of lane+1}
                M2 Y = A[0];
#pragma unroll
                for (int r = 1; r < R; ++r) Y = mul(A[r], Y);
                M2 tot;
                const M2 X = wave_suffix_product_excl(Y, lane, tot);
                // row vector c_n = C_sc A_{N-1} ... A_{n+1},  C_sc = [1, 1/eta]  (MPCSolver.cpp:375-379)
                const double ie = 1.0 / c.eta;
                double c0 = X.a + ie * X.c, c1 = X.b + ie * X.d;
#pragma unroll
                for (int r = R - 1; r >= 0; --r) {
                    a[r] = c0 * B0[r] + c1 * B1[r];                        // Aeq(n) = C_sc phi_input(:,n)
                    const double n0 = c0 * A[r].a + c1 * A[r].c, n1 = c0 * A[r].b + c1 * A[r].d;
                    c0 = n0; c1 = n1;
                }
                const double cps0 = tot.a + ie * tot.c, cps1 = tot.b + ie * tot.d;   // C_sc phi_state
                // ---- box midpoints and reductions
                const double h = (w.fc > 1) ? c.half_run : c.half_first;     // MPCSolver.cpp:328-338
                hbox = h;
                double aa[R];
                double s_abs = 0.0, s_ax = 0.0, s_ay = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int n = lane * R + r;
                    double mx = 0.0, my = 0.0;
                    if (n < N) { mx = c.midx[idx + n]; my = c.midy[idx + n]; } else a[r] = 0.0;
                    aa[r] = fabs(a[r]);
                    s_abs += aa[r]; s_ax += a[r] * mx; s_ay += a[r] * my;
                }
                s_abs = wave_sum(s_abs); s_ax = wave_sum(s_ax); s_ay = wave_sum(s_ay);
                const double beq_x = -(cps0 * x0 + cps1 * xd0) + c.tailx[idx];   // MPCSolver.cpp:381-384
                const double beq_y = -(cps0 * y0 + cps1 * yd0) + c.taily[idx];
                // v = u - mid:  sum a v = bp,  |v| <= h   ->  v_n = sg * sign(a_n) * min(tau |a_n|, h);
                // G(tau) = sum |a_n| min(tau |a_n|, h) is concave piecewise linear: Newton from tau = 0 is
                // monotone and lands on the exact breakpoint interval in a handful of steps.
                const double bpx = beq_x - s_ax, bpy = beq_y - s_ay;
                sgx = (bpx < 0.0) ? -1.0 : 1.0; sgy = (bpy < 0.0) ? -1.0 : 1.0;
                const double T[2] = { fabs(bpx), fabs(bpy) };
                const double gmax = h * s_abs;
                bool done[2]; int prev[2] = {-1, -1}, its[2] = {0, 0};
#pragma unroll
                for (int ax = 0; ax < 2; ++ax) {
                    const bool inf = T[ax] > gmax * (1.0 + 1e-12) + 1e-300;
                    if (inf) { status |= (ax == 0 ? ISMPC_ST_X_INFEASIBLE : ISMPC_ST_Y_INFEASIBLE); tau[ax] = INFINITY; }
                    done[ax] = inf;
                }
                for (int it = 0; it < N + 2 && !(done[0] && done[1]); ++it) {
                    double ssat[2] = {0.0, 0.0}, qfree[2] = {0.0, 0.0}; int cnt[2] = {0, 0};
#pragma unroll
                    for (int ax = 0; ax < 2; ++ax) {
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const bool sat = tau[ax] * aa[r] >= h;
                            ssat[ax] += sat ? aa[r] : 0.0;
                            qfree[ax] += sat ? 0.0 : a[r] * a[r];
                            cnt[ax] += __popcll(__builtin_amdgcn_ballot_w64(sat));
                        }
                    }
#pragma unroll
                    for (int ax = 0; ax < 2; ++ax) {
                        if (done[ax]) continue;
                        if (cnt[ax] == prev[ax]) { done[ax] = true; continue; }
                        const double ss = wave_sum(ssat[ax]), qf = wave_sum(qfree[ax]);
                        ++its[ax];
                        if (!(qf > 0.0)) { tau[ax] = INFINITY; done[ax] = true; continue; }
                        const double tn = (T[ax] - h * ss) / qf;
                        if (!(tn > tau[ax])) { done[ax] = true; continue; }
                        tau[ax] = tn; prev[ax] = cnt[ax];
                    }
                }
                itx = its[0]; ity = its[1];
                {   // first decision variables (lane 0 holds sample 0)
                    const double a0 = bcast0(a[0]), aa0 = fabs(a0), sa0 = (a0 < 0.0) ? -1.0 : 1.0;
                    const double m0x = c.midx[idx], m0y = c.midy[idx];
                    ux0 = m0x + sgx * sa0 * ((aa0 > 0.0) ? fmin(tau[0] * aa0, h) : 0.0);
                    uy0 = m0y + sgy * sa0 * ((aa0 > 0.0) ? fmin(tau[1] * aa0, h) : 0.0);
                }
            } else {
                status |= ISMPC_ST_FLIGHT;
            }
            // ---- integration with A(lambda_0), B(lambda_0), MPCSolver.cpp:406-422
            o_x  = (A0.a * x0 + A0.b * xd0) + B00 * ux0;
            o_xd = (A0.c * x0 + A0.d * xd0) + B10 * ux0;
            o_y  = (A0.a * y0 + A0.b * yd0) + B00 * uy0;
            o_yd = (A0.c * y0 + A0.d * yd0) + B10 * uy0;
        }

        const QOut o = {o_x, o_y, o_z, o_xd, o_yd, o_zd, uz0, ux0, uy0, status, itx, ity};
        store_record_lanes(out, gi, lane, o, 0);
        if (u_traj) {
            double* dst = u_traj + (size_t)gi * 3 * N;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = lane * R + r;
                if (n < N) {
                    double vx = 0.0, vy = 0.0;
                    if (stage3) {
                        const double aa = fabs(a[r]), sa = (a[r] < 0.0) ? -1.0 : 1.0;
                        vx = c.midx[idx + n] + sgx * sa * ((aa > 0.0) ? fmin(tau[0] * aa, hbox) : 0.0);
                        vy = c.midy[idx + n] + sgy * sa * ((aa > 0.0) ? fmin(tau[1] * aa, hbox) : 0.0);
                    }
                    dst[n] = u[r]; dst[N + n] = vx; dst[2 * N + n] = vy;
                }
            }
        }
        // ---- closed loop: feed back (Controller.cpp:346-348) and advance counters (:503-504)
        if (rollout_frame >= 0 && lane == 0) store_feedback(c, state_rw + gi, o, w);
    }
}

}  // namespace
