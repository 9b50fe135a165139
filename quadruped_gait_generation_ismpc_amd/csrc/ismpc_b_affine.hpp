// Formulation B, part 3 of 4 of the translation unit ismpc_hip.hip: one instance per wavefront.  The per-tick kernel of
// ISMPC_PATH=wave and of horizons 128 < N <= 256 (ismpc_tick_affine), the active-set solve of the vertical QP's inequality rows
// (z_active_set), and the forms in which the lane-group kernels reach that fallback: a second launch over the list of deferred
// instances (ismpc_tick_affine_fallback) or a call from inside their own launch (fallback_call, fallback_call_one).
#pragma once
#include "ismpc_b_common.hpp"

namespace {

// ======================================================================================
// Fast path: one wavefront = one instance, no LDS, no barrier.
// The vertical QP (MPCSolver.cpp:220-278) is evaluated from the affine tables (the dense solve
// happened once at ismpc_create); what is left per tick is the nonlinear part: lambda_j, the
// 2x2 suffix scan, and the two exact knapsack solves.
// ======================================================================================
template <int CTRL>
__device__ __forceinline__ double dpp64z(double src)        // DPP move, out-of-range source lanes read 0
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(src), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(src), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// y <- T y for T = I + Tm taken from another lane (Tm = 0 where that lane does not exist)
template <int CTRL>
__device__ __forceinline__ void scan_step(M2& y)
{
    const double ta = dpp64z<CTRL>(y.a - 1.0), tb = dpp64z<CTRL>(y.b), tc = dpp64z<CTRL>(y.c), td = dpp64z<CTRL>(y.d - 1.0);
    M2 r;
    r.a = fma(ta, y.a, fma(tb, y.c, y.a)); r.b = fma(ta, y.b, fma(tb, y.d, y.b));
    r.c = fma(tc, y.a, fma(td, y.c, y.c)); r.d = fma(tc, y.b, fma(td, y.d, y.d));
    y = r;
}
template <int R> __device__ __forceinline__ void loadR(const double* p, double (&v)[R])
{
    if constexpr (R == 2) { const double2 t = *reinterpret_cast<const double2*>(p); v[0] = t.x; v[1] = t.y; }
    else if constexpr (R == 4) { const double2 t = *reinterpret_cast<const double2*>(p), q = *reinterpret_cast<const double2*>(p + 2); v[0] = t.x; v[1] = t.y; v[2] = q.x; v[3] = q.y; }
    else {
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = p[r];
    }
}

// ---- vertical QP with active inequality rows (MPCSolver.cpp:158-160: 0 <= S_bar_z u <= 1e4), rare path ----
// Dual active-set (Goldfarb-Idnani step logic) in range-space form over the inequality rows only: the equalities are
// already inside the reduced inverse P_p = (I - W_p E_p') Hinv, so with p_k = P_p S_k' and g_k = S p_k (rows of the HSt /
// SHSt tables, pattern folded in with Wt / SW) the Gram matrix of the working set is G[j][k] = g_k[row_j].
// The working set may grow to every row of the horizon (the reference's solver, utils.cpp:264-383, has no cap either), so
// G^-1 (q x q) and the per-entry vectors live in a slot of a handle-owned pool in HBM; one wavefront owns a slot while it
// solves.  Nothing here is on the hot path: the nominal and perturbed gait workloads never activate a row.
__device__ __forceinline__ double readlane_dyn(double v, int l)
{
    const int ll = __builtin_amdgcn_readfirstlane(l);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), ll), __builtin_amdgcn_readlane(__double2loint(v), ll));
}
__device__ __forceinline__ int readlane_dyn(int v, int l) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ double wave_allmax(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_allmin(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_allmin_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
template <int R>
__device__ __forceinline__ double sample_at(const double (&v)[R], int k)     // v at sample k (k wave-uniform)
{
    const int owner = k / R, slot = k - owner * R;
    double x = v[0];
#pragma unroll
    for (int r = 1; r < R; ++r) if (slot == r) x = v[r];
    return readlane_dyn(x, owner);
}
// Folds the equality pattern into a row of (HSt, SHSt) or into a combination of such rows: p -= W_e ue_e, g -= (S W)_e ue_e with
// ue_e = the UNPROJECTED vector at the e-th pinned sample (lane e holds it in `uel`); the pinned samples of p end up zero.
template <int R>
__device__ __forceinline__ void z_project(const DevConst& c, int n0, int pat, int elo, int ne, double uel, double (&pc)[R], double (&gc)[R])
{
    constexpr int NT = ismpc::Tables::NT;
    for (int e = 0; e < ne; ++e) {                       // (not unrolled: the lane read is a convergent operation)
        const double ue = readlane_dyn(uel, e);
        double wv[R], sv[R];
        loadR<R>(c.Wt + ((size_t)pat * c.Fmax + e) * NT + n0, wv); loadR<R>(c.SW + ((size_t)pat * c.Fmax + e) * NT + n0, sv);
#pragma unroll
        for (int r = 0; r < R; ++r) { pc[r] = fma(-wv[r], ue, pc[r]); gc[r] = fma(-sv[r], ue, gc[r]); }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { const int n = n0 + r; if (n >= elo && n < elo + ne) pc[r] = 0.0; }
}
template <int R>
__device__ __forceinline__ void z_fetch(const DevConst& c, int lane, int row, int n0, int pat, int elo, int ne, double (&pc)[R], double (&gc)[R])
{
    constexpr int NT = ismpc::Tables::NT;
    loadR<R>(c.HSt + (size_t)row * NT + n0, pc); loadR<R>(c.SHSt + (size_t)row * NT + n0, gc);
    const double uel = (lane < ne) ? c.HSt[(size_t)row * NT + elo + lane] : 0.0;
    z_project<R>(c, n0, pat, elo, ne, uel, pc, gc);
}
// one wavefront's stores to its working storage become visible to its other lanes (same CU: a wait for the stores is all it takes)
#define Z_MEMSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

// A slot of the pool: lane 0 takes the first free one starting at `hint`.  Holders always finish (bounded iteration
// count) and wait for nobody, so spinning here cannot deadlock, whatever is resident.
__device__ __forceinline__ int z_slot_acquire(const DevConst& c, int lane, int hint)
{
    int s = 0;
    if (lane == 0) {
        s = (int)((unsigned)hint % (unsigned)c.zslots);
        while (atomicCAS(&c.zbusy[s], 0, 1) != 0) { s = (s + 1 == c.zslots) ? 0 : s + 1; __builtin_amdgcn_s_sleep(8); }
    }
    s = __builtin_amdgcn_readfirstlane(s);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return s;
}
__device__ __forceinline__ void z_slot_release(const DevConst& c, int lane, int slot)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) atomicExch(&c.zbusy[slot], 0);
}

// Working storage of one solve: G^-1 (ld x ld), the per-entry vectors, g of the entering row by sample, the entries' rows.
// Up to Z_LDS_Q entries it is the wavefront's own LDS window (Z_LDS_DOUBLES doubles, handed in by the kernel); a working set
// that outgrows it moves to a slot of the pool in HBM (ld = zcap) and stays there.  The pointers are wave-uniform and generic.
constexpr int Z_LDS_Q = 16;
constexpr int Z_LDS_DOUBLES = Z_LDS_Q * Z_LDS_Q + 4 * Z_LDS_Q + ismpc::Tables::NT + Z_LDS_Q / 2;
struct ZStore {
    double *Ginv, *amu, *asg, *rv, *dv, *gs; int* arow; int ld;
    __device__ __forceinline__ void bind(double* base, int ld_)
    {
        Ginv = base; ld = ld_; amu = base + (size_t)ld_ * ld_; asg = amu + ld_; rv = asg + ld_; dv = rv + ld_; gs = dv + ld_;
        arow = reinterpret_cast<int*>(gs + ismpc::Tables::NT);
    }
};

// returns the iteration count; updates u, su in place.  Entry j of the working set: row arow[j], bound sign asg[j] (+1 lower,
// -1 upper), multiplier amu[j]; Ginv = G^-1 over the entries.
template <int R>
__device__ int z_active_set(const DevConst& c, int lane, int n0, int pat, double (&u)[R], double (&su)[R], int& status, int slot_hint, double* lds)
{
    constexpr int NT = ismpc::Tables::NT;
    const int N = c.N, cap = c.zcap;
    int elo = 0, ne = 0;
    if (pat < c.npat) { elo = c.e_lo[pat]; ne = c.ne[pat]; }
    const double tol_lo = z_tol(c.z_lo), tol_hi = z_tol(c.z_hi);
    ZStore z; z.bind(lds, c.zldsq);
    int slot = -1;
    bool sact[R];
#pragma unroll
    for (int r = 0; r < R; ++r) sact[r] = false;
    int q = 0, its = 0;
    const int max_its = 8 * N + 64;
    Z_MEMSYNC();                                             // whatever the caller kept in the window has been read
    for (;;) {
        // ---- most violated free row
        double best = 0.0; int code = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = n0 + r;
            if (n < N && !sact[r]) {
                const double vl = c.z_lo - su[r], vh = su[r] - c.z_hi;
                if (vl > tol_lo && vl > best) { best = vl; code = 2 * n; }
                if (vh > tol_hi && vh > best) { best = vh; code = 2 * n + 1; }
            }
        }
        const double vmax = wave_allmax(best);
        if (!(vmax > 0.0)) break;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(best == vmax);
        code = readlane_dyn(code, (int)__builtin_ctzll(m));
        const int row = code >> 1;
        const double sg = (code & 1) ? -1.0 : 1.0;
        if (q >= cap) { status |= ISMPC_ST_Z_FAILED; break; }             // cannot happen: entries are distinct rows, cap = N
        if (q == z.ld && slot < 0) {
            // ---- the working set outgrows the LDS window: everything moves to a pool slot
            slot = z_slot_acquire(c, lane, slot_hint);
            ZStore zp; zp.bind(c.zpool + (size_t)slot * c.zstride, cap);
#pragma nounroll
            for (int j = lane; j < q; j += 64) {
#pragma nounroll
                for (int k = 0; k < q; ++k) zp.Ginv[(size_t)k * cap + j] = z.Ginv[k * z.ld + j];
                zp.amu[j] = z.amu[j]; zp.asg[j] = z.asg[j]; zp.arow[j] = z.arow[j];
            }
            z = zp;
            Z_MEMSYNC();
        }
        double* const Ginv = z.Ginv; double* const amu = z.amu; double* const asg = z.asg; double* const rv = z.rv; double* const dv = z.dv;
        double* const gs = z.gs; int* const arow = z.arow;
        const size_t ld = (size_t)z.ld;
        double pc[R], gc[R];
        z_fetch<R>(c, lane, row, n0, pat, elo, ne, pc, gc);
        const double npn = sample_at<R>(gc, row);
#pragma unroll
        for (int r = 0; r < R; ++r) if (n0 + r < NT) gs[n0 + r] = gc[r];
        Z_MEMSYNC();
        double mu_p = 0.0;
        bool fail = false;
        for (;;) {
            if (++its > max_its) { fail = true; break; }
            const double srow = sample_at<R>(su, row);
            const double sviol = sg > 0.0 ? srow - c.z_lo : c.z_hi - srow;
            // d_j = sg * asg_j * g_row[arow_j] ;  r = G^-1 d ;  ratio test over the entries
#pragma nounroll
            for (int j = lane; j < q; j += 64) dv[j] = sg * asg[j] * gs[arow[j]];
            Z_MEMSYNC();
            double drl = 0.0, tcl = INFINITY; int tl = 1 << 30;
#pragma nounroll
            for (int j = lane; j < q; j += 64) {
                double acc = 0.0;
#pragma unroll 4
                for (int k = 0; k < q; ++k) acc = fma(Ginv[(size_t)k * ld + j], dv[k], acc);        // column j = row j (symmetric)
                rv[j] = acc; drl = fma(dv[j], acc, drl);
                if (acc > 0.0) { const double tt = amu[j] / acc; if (tt < tcl) { tcl = tt; tl = j; } }
            }
            Z_MEMSYNC();
            const double gamma = npn - wave_sum(drl);
            const double t1 = wave_allmin(tcl);
            const double t2 = (gamma > 1e-12 * npn) ? -sviol / gamma : INFINITY;
            const double t = fmin(t1, t2);
            if (!(t < INFINITY)) { fail = true; break; }
            if (t2 < INFINITY) {
                // z = P (n+ - N r): the entries' rows of (HSt, SHSt) combined with coefficient -r_j asg_j (independent loads, four
                // in flight), the equality pattern folded into the combination ONCE (it is linear), plus the new row
                double zu[R], zs[R], vu[R], vs[R];
#pragma unroll
                for (int r = 0; r < R; ++r) { vu[r] = 0.0; vs[r] = 0.0; }
                double uel = 0.0;
#pragma unroll 4
                for (int j = 0; j < q; ++j) {
                    const double cf = -rv[j] * asg[j];
                    const size_t rj = (size_t)arow[j] * NT;
                    double pj[R], gj[R];
                    loadR<R>(c.HSt + rj + n0, pj); loadR<R>(c.SHSt + rj + n0, gj);
                    const double uj = (lane < ne) ? c.HSt[rj + elo + lane] : 0.0;
                    uel = fma(cf, uj, uel);
#pragma unroll
                    for (int r = 0; r < R; ++r) { vu[r] = fma(cf, pj[r], vu[r]); vs[r] = fma(cf, gj[r], vs[r]); }
                }
                if (q > 0) z_project<R>(c, n0, pat, elo, ne, uel, vu, vs);
#pragma unroll
                for (int r = 0; r < R; ++r) { zu[r] = fma(sg, pc[r], vu[r]); zs[r] = fma(sg, gc[r], vs[r]); }
#pragma unroll
                for (int r = 0; r < R; ++r) { u[r] = fma(t, zu[r], u[r]); su[r] = fma(t, zs[r], su[r]); }
            }
#pragma nounroll
            for (int j = lane; j < q; j += 64) amu[j] -= t * rv[j];
            mu_p += t;
            if (t2 < INFINITY && t == t2) {
                // ---- the row enters: border update of G^-1
                const double ig = 1.0 / gamma;
#pragma nounroll
                for (int j = lane; j < q; j += 64) {
                    const double rj = rv[j];
#pragma unroll 4
                    for (int k = 0; k < q; ++k) Ginv[(size_t)k * ld + j] = fma(rv[k] * ig, rj, Ginv[(size_t)k * ld + j]);
                    Ginv[(size_t)q * ld + j] = -rj * ig; Ginv[(size_t)j * ld + q] = -rj * ig;
                }
                if (lane == 0) { Ginv[(size_t)q * ld + q] = ig; arow[q] = row; asg[q] = sg; amu[q] = mu_p; }
#pragma unroll
                for (int r = 0; r < R; ++r) if (n0 + r == row) sact[r] = true;
                ++q;
                Z_MEMSYNC();
                break;
            }
            // ---- entry l (the first one attaining t1) leaves: Schur update, the last entry moves into its place
            Z_MEMSYNC();
            const int l = wave_allmin_i((tcl == t1) ? tl : (1 << 30));
            const int last = q - 1;
            const int drow = arow[l];
            const double piv = Ginv[(size_t)l * ld + l];
#pragma nounroll
            for (int j = lane; j < q; j += 64) rv[j] = Ginv[(size_t)l * ld + j];                    // column l
            Z_MEMSYNC();
#pragma nounroll
            for (int j = lane; j < q; j += 64) {
                if (j == l) continue;
                const double cj = rv[j] / piv;
#pragma nounroll
                for (int k = 0; k < q; ++k) if (k != l) Ginv[(size_t)k * ld + j] -= rv[k] * cj;
            }
            Z_MEMSYNC();
            if (l != last) {
#pragma nounroll
                for (int j = lane; j < q; j += 64) {
                    if (j == l) continue;
                    const double vl_ = Ginv[(size_t)last * ld + j];
                    Ginv[(size_t)l * ld + j] = vl_; Ginv[(size_t)j * ld + l] = vl_;
                }
                Z_MEMSYNC();
                if (lane == 0) { Ginv[(size_t)l * ld + l] = Ginv[(size_t)last * ld + last]; arow[l] = arow[last]; asg[l] = asg[last]; amu[l] = amu[last]; }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) if (n0 + r == drow) sact[r] = false;
            --q;
            Z_MEMSYNC();
        }
        if (fail) { status |= ISMPC_ST_Z_FAILED; break; }
    }
    if (slot >= 0) z_slot_release(c, lane, slot);
    Z_MEMSYNC();                                             // the window is the caller's again
    return its;
}

template <int R, bool FB>
__device__ __forceinline__ void tick_affine_body(const DevConst& c, const int gi, const int lane,
                                                 const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                                                 ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj,
                                                 int rollout_frame, unsigned char* zmark, int launch_id, int* zlist = nullptr, int zbatch = 0, double* zlds = nullptr,
                                                 const int extra_status = 0)
{
    constexpr int NT = ismpc::Tables::NT;
    const int N = c.N;
    bool deferred = false;                            // FB == false: an instance with active inequality rows is left to the fallback kernel
    const double dt = c.dt;
    const ismpc_tick_in* rec = ((rollout_frame >= 0) ? state_rw : in_ro) + gi;
    const Walk w = load_walk(c, rec, rollout_frame);
    const double x0 = rec->com_pos[0], y0 = rec->com_pos[1], z0 = rec->com_pos[2];
    const double xd0 = rec->com_vel[0], yd0 = rec->com_vel[1], zd0 = rec->com_vel[2];
    int idx;
    int status = gate_tick(c, w, idx) | extra_status;       // (extra_status: a sweep instance that names no parameter set -- passed through)
    double o_x = x0, o_y = y0, o_z = z0, o_xd = xd0, o_yd = yd0, o_zd = zd0;
    double uz0 = 0.0, ux0 = 0.0, uy0 = 0.0;
    int itx = 0, ity = 0, zits = 0;
    const int n0 = lane * R;                          // this lane owns samples n0 .. n0+R-1 (tables are zero past N)
    double u[R], a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { u[r] = 0.0; a[r] = 0.0; }
    double tau0 = 0.0, tau1 = 0.0, sgx = 1.0, sgy = 1.0, hbox = 0.0;
    bool stage3 = false;

    if (status == 0) {
        // ---- vertical stage from the affine tables; pattern = which u_i = 0 rows are present
        // (MPCSolver.cpp:223-243, is_running :262-263)
        const int pat = (w.fc > 1 && w.mpc < c.npat) ? w.mpc : c.npat;
        const double* T = c.vtab + (size_t)pat * 6 * NT + n0;
        double t0[R], t1[R], t2[R], su[R], tz[R], tg[R];
        loadR<R>(T, t0); loadR<R>(T + NT, t1); loadR<R>(T + 2 * NT, t2);
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = fma(zd0, t2[r], fma(z0, t1[r], t0[r]));
        loadR<R>(T + 3 * NT, t0); loadR<R>(T + 4 * NT, t1); loadR<R>(T + 5 * NT, t2);
#pragma unroll
        for (int r = 0; r < R; ++r) su[r] = fma(zd0, t2[r], fma(z0, t1[r], t0[r]));
        loadR<R>(c.tz + n0, tz); loadR<R>(c.tg + n0, tg);
        if (!c.flat) {                                  // plans with mid_z != 0 (MPCSolver.cpp:259)
            double du[R], ds[R];
            loadR<R>(c.dU + (size_t)idx * NT + n0, du); loadR<R>(c.SdU + (size_t)idx * NT + n0, ds);
            int elo = 0, ne = 0;
            if (pat < c.npat) { elo = c.e_lo[pat]; ne = c.ne[pat]; }
            for (int e = 0; e < ne; ++e) {
                const double ue = c.dU[(size_t)idx * NT + elo + e];
                double wv[R], sv[R];
                loadR<R>(c.Wt + ((size_t)pat * c.Fmax + e) * NT + n0, wv); loadR<R>(c.SW + ((size_t)pat * c.Fmax + e) * NT + n0, sv);
#pragma unroll
                for (int r = 0; r < R; ++r) { du[r] = fma(-wv[r], ue, du[r]); ds[r] = fma(-sv[r], ue, ds[r]); }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = n0 + r;
                u[r] += du[r]; su[r] += ds[r];
                if (n >= elo && n < elo + ne) u[r] = 0.0;
            }
        }
        bool viol = false;
        double lam[R];
        const double zlo_t = c.z_lo - z_tol(c.z_lo), zhi_t = c.z_hi + z_tol(c.z_hi);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = n0 + r;
            viol = viol || (n < N && (su[r] < zlo_t || su[r] > zhi_t));         // MPCSolver.cpp:158-160, beyond rounding
        }
        const bool anyviol = __builtin_amdgcn_ballot_w64(viol) != 0;
        if (anyviol) {
            status |= ISMPC_ST_Z_INEQ_ACTIVE;
            if constexpr (FB) zits = z_active_set<R>(c, lane, n0, pat, u, su, status, gi, zlds);
            else deferred = true;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double zpos = su[r] + fma(tz[r], zd0, z0) + tg[r];            // S u + T_bar_z s + T_bar_g_z
            const double zacc = fma(c.inv_mass, u[r], -c.g);
            lam[r] = (c.g + zacc) * frcp(zpos);                                 // MPCSolver.cpp:306
        }
        uz0 = bcast0(u[0]);
        integrate_z(c, c.dt_over_mass, c.h_des, z0, zd0, uz0, o_z, o_zd, status);

        // ---- A_j, B_j (MPCSolver.cpp:353-361): A = [1+wQ, dt P; lam dt P, 1+wQ], B = [-wQ, -lam dt P]
        double ch1[R], s1[R], s2[R];
        bool big = false, mid = false;
        double wv_[R], le_[R], dtn_[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = n0 + r;
            le_[r] = (lam[r] < c.gate) ? 0.0 : lam[r];
            dtn_[r] = (n < N) ? dt : 0.0;
            wv_[r] = le_[r] * dtn_[r] * dtn_[r];
            big = big || (wv_[r] > 0.25);
            mid = mid || (wv_[r] > 0.004);
        }
        // degree 3 where every lane's w allows it (taylor_low); the wave takes degree 7 only if some lane needs it
        if (__builtin_amdgcn_ballot_w64(mid) == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double P = TAYLOR_P3, Q = TAYLOR_Q3;
                taylor_low(wv_[r], P, Q);
                ab_series(wv_[r], dtn_[r], le_[r], P, Q, ch1[r], s1[r], s2[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double P, Q;
                taylor_high(wv_[r], P, Q); taylor_low(wv_[r], P, Q);
                ab_series(wv_[r], dtn_[r], le_[r], P, Q, ch1[r], s1[r], s2[r]);
            }
        }
        if (__builtin_amdgcn_ballot_w64(big) != 0) {      // lambda dt^2 > 1/4: off any physical gait; libm, wave-uniform
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (wv_[r] > 0.25) ab_libm(wv_[r], dtn_[r], le_[r], ch1[r], s1[r], s2[r]);
        }
        const double lam0 = bcast0(lam[0]);
        const double A0a = 1.0 + bcast0(ch1[0]), A0b = bcast0(s1[0]), A0c = bcast0(s2[0]);

        if (lam0 > c.gate) {                                                    // MPCSolver.cpp:322
            stage3 = true;
            // ---- inclusive suffix product over lanes: Y_L = A(block 63) ... A(block L), row by row
            M2 Y = (M2){1.0 + ch1[0], s1[0], s2[0], 1.0 + ch1[0]};
#pragma unroll
            for (int r = 1; r < R; ++r) Y = mul((M2){1.0 + ch1[r], s1[r], s2[r], 1.0 + ch1[r]}, Y);
            scan_step<0x101>(Y); scan_step<0x102>(Y); scan_step<0x104>(Y); scan_step<0x108>(Y);   // row_shl 1,2,4,8
            // g_row = C_sc P_3 .. P_{row+1}  (P_r = product of row r = Y at its first lane), C_sc = [1, 1/eta]
            const double ie = c.inv_eta;
            const M2 p1 = readlane_m2<16>(Y), p2 = readlane_m2<32>(Y), p3 = readlane_m2<48>(Y);
            const double g2a = fma(ie, p3.c, p3.a), g2b = fma(ie, p3.d, p3.b);
            const double g1a = fma(g2b, p2.c, g2a * p2.a), g1b = fma(g2b, p2.d, g2a * p2.b);
            const double g0a = fma(g1b, p1.c, g1a * p1.a), g0b = fma(g1b, p1.d, g1a * p1.b);
            const int row = lane >> 4;
            const double ga = row == 3 ? 1.0 : (row == 2 ? g2a : (row == 1 ? g1a : g0a));
            const double gb = row == 3 ? ie  : (row == 2 ? g2b : (row == 1 ? g1b : g0b));
            // cv_L = C_sc (suffix product from the first sample of lane L) ; the lane needs it one lane up
            const double cva = fma(gb, Y.c, ga * Y.a), cvb = fma(gb, Y.d, ga * Y.b);
            const double cps0 = readlane64<0>(cva), cps1 = readlane64<0>(cvb);  // C_sc phi_state
            double c0 = dppv<0x130, 0xf, false>(1.0, cva), c1 = dppv<0x130, 0xf, false>(ie, cvb);   // wave_shl:1
            // ---- Aeq(n) = C_sc phi_input(:,n) = c_n B_n, walking the lane's samples backwards
#pragma unroll
            for (int r = R - 1; r >= 0; --r) {
                a[r] = -fma(c0, ch1[r], c1 * s2[r]);
                const double k0 = fma(c0, ch1[r], fma(c1, s2[r], c0)), k1 = fma(c1, ch1[r], fma(c0, s1[r], c1));
                c0 = k0; c1 = k1;
            }
            const double h = (w.fc > 1) ? c.half_run : c.half_first;            // MPCSolver.cpp:328-338
            hbox = h;
            double q0 = 0.0, s_ax = 0.0, s_ay = 0.0;
            double mx[R], my[R];                          // loaded here, not earlier: 8 waves per SIMD hide the latency, registers are the scarce resource
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = n0 + r;
                mx[r] = (n < N) ? c.midx[idx + n] : 0.0; my[r] = (n < N) ? c.midy[idx + n] : 0.0;
            }
            const double tailx = c.tailx[idx], taily = c.taily[idx];
#pragma unroll
            for (int r = 0; r < R; ++r) { q0 = fma(a[r], a[r], q0); s_ax = fma(a[r], mx[r], s_ax); s_ay = fma(a[r], my[r], s_ay); }
            q0 = wave_sum(q0); s_ax = wave_sum(s_ax); s_ay = wave_sum(s_ay);
            const double bpx = (tailx - fma(cps0, x0, cps1 * xd0)) - s_ax;      // beq - a'mid, MPCSolver.cpp:381-384
            const double bpy = (taily - fma(cps0, y0, cps1 * yd0)) - s_ay;
            sgx = (bpx < 0.0) ? -1.0 : 1.0; sgy = (bpy < 0.0) ? -1.0 : 1.0;
            // min 1/2|v|^2, a'v = bp, |v| <= h  ->  v_n = sg sign(a_n) min(tau |a_n|, h): Newton on the concave
            // piecewise-linear G(tau) = sum |a_n| min(tau |a_n|, h) from tau = 0 (first step: tau = |bp| / sum a^2)
            const double T[2] = { fabs(bpx), fabs(bpy) };
            const double iq0 = frcp(q0);
            double tau[2] = { T[0] * iq0, T[1] * iq0 };
            int its[2] = {1, 1};
            double aa[R];
#pragma unroll
            for (int r = 0; r < R; ++r) aa[r] = fabs(a[r]);
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) {
                if (!(q0 > 0.0)) {                                               // no sample can move the ZMP
                    tau[ax] = (T[ax] > 0.0) ? INFINITY : 0.0;
                    if (T[ax] > 1e-300) status |= (ax == 0 ? ISMPC_ST_X_INFEASIBLE : ISMPC_ST_Y_INFEASIBLE);
                }
                int prev = 0;
                for (int it = 0; it < N + 2; ++it) {
                    int cnt = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r) cnt += __popcll(__builtin_amdgcn_ballot_w64(tau[ax] * aa[r] >= h));
                    if (cnt == prev) break;                                      // active set unchanged: exact
                    double ssat = 0.0, qfree = 0.0;
#pragma unroll
                    for (int r = 0; r < R; ++r) { const bool sat = tau[ax] * aa[r] >= h; ssat += sat ? aa[r] : 0.0; const double a2 = a[r] * a[r]; qfree += sat ? 0.0 : a2; }
                    ssat = wave_sum(ssat); qfree = wave_sum(qfree);
                    ++its[ax];
                    const double rem = fma(-h, ssat, T[ax]);
                    if (!(qfree > 0.0)) {                                        // everything saturated
                        if (rem > fma(h * ssat, 1e-12, 1e-300)) status |= (ax == 0 ? ISMPC_ST_X_INFEASIBLE : ISMPC_ST_Y_INFEASIBLE);
                        tau[ax] = INFINITY; break;
                    }
                    const double tn = rem * frcp(qfree);
                    if (!(tn > tau[ax])) break;
                    tau[ax] = tn; prev = cnt;
                }
            }
            tau0 = tau[0]; tau1 = tau[1]; itx = its[0]; ity = its[1];
            {   // first decision variables (lane 0 holds sample 0)
                const double a0 = bcast0(a[0]);
                ux0 = box_move(sgx, a0, tau0, h, bcast0(mx[0]));
                uy0 = box_move(sgy, a0, tau1, h, bcast0(my[0]));
            }
        } else {
            status |= ISMPC_ST_FLIGHT;
        }
        // ---- integration with A(lambda_0), B(lambda_0), MPCSolver.cpp:406-422
        integrate_xy(A0a, A0b, A0c, x0, xd0, ux0, o_x, o_xd);
        integrate_xy(A0a, A0b, A0c, y0, yd0, uy0, o_y, o_yd);
    }

    const QOut o = {o_x, o_y, o_z, o_xd, o_yd, o_zd, uz0, ux0, uy0, status, itx, ity};
    store_record_lanes(out, gi, lane, o, zits);
    if (u_traj) {
        double* dst = u_traj + (size_t)gi * 3 * N;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = n0 + r;
            if (n < N) {
                double vx = 0.0, vy = 0.0;
                if (stage3) { vx = box_move(sgx, a[r], tau0, hbox, c.midx[idx + n]); vy = box_move(sgy, a[r], tau1, hbox, c.midy[idx + n]); }
                dst[n] = u[r]; dst[N + n] = vx; dst[2 * N + n] = vy;
            }
        }
    }
    // ---- closed loop: feed back (Controller.cpp:346-348) and advance counters (:503-504)
    if constexpr (!FB) {
        if (deferred && lane == 0 && zlist) {
            const int slot = atomicAdd(c.zflag, 1);
            if (slot < zbatch) zlist[slot] = gi;            // (an instance appends once per step and the count starts at 0: always true)
        }
    }
    if (rollout_frame >= 0 && lane == 0 && !deferred && !(status & ISMPC_ST_Z_FAILED)) store_feedback(c, state_rw + gi, o, w);   // a failed vertical solve is flagged, never fed back
}


// 8 workgroups (one wavefront per SIMD each) must be co-resident per CU: <= 64 VGPRs and -- the binding one on
// gfx950 -- <= 80 SGPRs (MI355X_MICROARCH.md "Residency": floor(800 / (ceil(sgpr/16)*16 + 16)) blocks per CU)
#ifndef ISMPC_AFF_WAVES
#define ISMPC_AFF_WAVES 4
#endif
// SW: a parameter-sweep handle at a horizon the lane-group kernels do not cover (128 < N <= 256): one instance per wavefront, so the
// instance's parameter set is wave-uniform and the body runs on that set's own record (tables and scalars), as the fallback launch does.
template <int R, int SW = 0>
__global__ __launch_bounds__(64 * ISMPC_AFF_WAVES) __attribute__((amdgpu_num_sgpr(80)))
void ismpc_tick_affine(const DevConst c, const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                       ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj, int batch, int rollout_frame,
                       unsigned char* zmark, int launch_id)
{
    const int lane = threadIdx.x & 63;
    const int gi = blockIdx.x * ISMPC_AFF_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (gi >= batch) return;
    if constexpr (SW) {
        int ps = __builtin_amdgcn_readfirstlane((((rollout_frame >= 0) ? state_rw : in_ro) + gi)->reserved);
        if constexpr (SW == 2) ps = record_index<2>(c, ps);          // (a multi-plan handle: the record of the instance's (set, plan) pair)
        const bool known = ps >= 0 && ps < c.nsets * (SW == 2 ? c.nplans : 1);   // an unknown set: ISMPC_ST_BAD_INDEX, state passed through
        tick_affine_body<R, false>(c.sets[known ? ps : 0], gi, lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id,
                                   zmark ? zlist_of(zmark, batch) : nullptr, batch, nullptr, known ? 0 : ISMPC_ST_BAD_INDEX);
    } else
    tick_affine_body<R, false>(c, gi, lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, zmark ? zlist_of(zmark, batch) : nullptr, batch);
}

// Second launch of every tick of a large batch: exits at once unless the first one deferred instances (active inequality rows).
template <int R, int SW = 0>
__global__ __launch_bounds__(256)
void ismpc_tick_affine_fallback(const DevConst c, const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                                ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj, int batch, int rollout_frame,
                                unsigned char* zmark, int launch_id)
{
    const int* zl = zlist_of(zmark, batch);
    const int ndef = min(*(volatile int*)c.zflag, batch);     // stable while this launch runs (the appending kernel is done): workgroup-uniform
    if (ndef == 0) return;
    __shared__ double zlds[4][Z_LDS_DOUBLES];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave0 = blockIdx.x * 4 + wv;
    double* const zwin = zlds[wv];
    for (int k = wave0; k < ndef; k += gridDim.x * 4) {
        const int gi = __builtin_amdgcn_readfirstlane(zl[k]);
        {
            if (SW) {
                // one instance per wavefront: its parameter set is wave-uniform, the body runs on that set's own record
                int ps = __builtin_amdgcn_readfirstlane((((rollout_frame >= 0) ? state_rw : in_ro) + gi)->reserved);
                if constexpr (SW == 2) ps = record_index<2>(c, ps);
                tick_affine_body<R, true>(c.sets[ps], gi, lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, nullptr, 0, zwin);    // (a deferred instance has a valid set)
            } else tick_affine_body<R, true>(c, gi, lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, nullptr, 0, zwin);
        }
    }
    // every workgroup has read the count by the time it gets here; the last one to arrive hands the counters back zeroed
    __syncthreads();
    if (threadIdx.x == 0 && atomicAdd(c.zflag + 1, 1) == (int)gridDim.x - 1) { c.zflag[0] = 0; c.zflag[1] = 0; __threadfence(); }
}

// The inequality fallback as a real CALL from the one-launch kernel: inlined there, its 200 registers' worth of state made the
// hot path of every tick spill 180 scalar registers; called, the tick keeps the register allocation of ismpc_tick_quad and only a
// wavefront that does defer an instance pays for the call.
template <int RW>
__device__ __attribute__((noinline)) void fallback_call(const DevConst* cp, int gi, int lane, const ismpc_tick_in* in_ro, ismpc_tick_in* state_rw,
                                                        ismpc_tick_out* out, double* u_traj, int rollout_frame, unsigned char* zmark, int launch_id, double* zlds)
{
    tick_affine_body<RW, true>(*cp, gi, lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, nullptr, 0, zlds);
}
// The same call from ismpc_tick_quad_one (ismpc_b_group.hpp, where one_occ() gives OCC):
template <int RW, int OCC>        // OCC: one copy per residency target (the register budget comes down from the calling kernels)
__device__ __attribute__((noinline))
void fallback_call_one(const DevConst* cp, int gi, int lane, const ismpc_tick_in* in_ro, ismpc_tick_in* state_rw,
                       ismpc_tick_out* out, double* u_traj, int rollout_frame, unsigned char* zmark, int launch_id, double* zlds)
{
    tick_affine_body<RW, true>(*cp, gi, lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, nullptr, 0, zlds);
}

}  // namespace
