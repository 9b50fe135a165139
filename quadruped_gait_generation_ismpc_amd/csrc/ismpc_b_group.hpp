// Formulation B, part 4 of 4 of the translation unit ismpc_hip.hip: the lane-group family, the default for horizons N <= 128.
// Per-tick kernels ismpc_tick_quad (two-launch form, with ismpc_tick_affine_fallback behind it), ismpc_tick_quad_inline and
// ismpc_tick_quad_one (one launch per step), the closed loop inside one launch (ismpc_rollout_quad), and the counting sort of
// ismpc_sweep_bind (sweep_sort_*).
#pragma once
#include "ismpc_b_affine.hpp"

namespace {

// =====================================================================================================================
// SEVERAL instances per wavefront, one group of LPI lanes each (horizons N <= 128): LPI = 16 (a DPP row, four instances per
// wavefront) or LPI = 8 (half a row, eight instances).  A horizon of 100 samples fills only 100 of the 128 sample slots of a
// wavefront and, worse, every scan, reduction and scalar of the tick is paid once per wavefront: with one instance per lane
// group the R = ceil(N/LPI) samples a lane owns are independent work for the FP64 pipe, the scans / reductions are log2(LPI)
// DPP steps inside a group (no cross-row fold, no readlane), and what used to be wave-uniform is group-uniform.  Same
// arithmetic as tick_affine_body; instances whose vertical QP has active inequality rows are deferred exactly as there.
template <int CTRL, int BANK_MASK>
__device__ __forceinline__ double dpp64b(double old, double src)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANK_MASK, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANK_MASK, false);
    return __hiloint2double(hi, lo);
}
// DPP move that writes every lane (rotations; shifts with bound_ctrl): no "old" operand, so no register to pre-load
template <int CTRL, bool BOUND_ZERO>
__device__ __forceinline__ double dpp64n(double src)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(src), CTRL, 0xf, 0xf, BOUND_ZERO);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(src), CTRL, 0xf, 0xf, BOUND_ZERO);
    return __hiloint2double(hi, lo);
}
// Lane-group primitives.  LPI = 16: the group is a DPP row.  LPI = 8: two groups per row; a shift by 4 is confined to its
// half row with the bank mask (banks 1 and 3 keep the zero / the old value), shifts by 1 and 2 zero the lanes whose source
// sits in the neighbouring group; sums are xor butterflies (quad_perm, quad_perm, row_half_mirror).
template <int LPI> struct Grp;
template <> struct Grp<16> {
    static constexpr int STEPS = 4;
    __device__ static __forceinline__ double sum(double v)             // sum over the group, in every lane (row_ror:1,2,4,8)
    {
        v += dpp64n<0x121, false>(v); v += dpp64n<0x122, false>(v); v += dpp64n<0x124, false>(v); v += dpp64n<0x128, false>(v);
        return v;
    }
    __device__ static __forceinline__ int sum_i(int v)
    {
        v += __builtin_amdgcn_mov_dpp(v, 0x121, 0xf, 0xf, false); v += __builtin_amdgcn_mov_dpp(v, 0x122, 0xf, 0xf, false);
        v += __builtin_amdgcn_mov_dpp(v, 0x124, 0xf, 0xf, false); v += __builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, false);
        return v;
    }
    // v from lane + 2^K of the group, 0 past its end
    template <int K> __device__ static __forceinline__ double shl0(double v, int) { return dpp64n<0x100 + (1 << K), true>(v); }
    // lane 0 of the group, in every lane: quad_perm [0,0,0,0], then row_shr:4 into bank 1, row_shr:8 into banks 2,3
    __device__ static __forceinline__ double bcast0(double v)
    {
        v = dpp64b<0x000, 0xf>(v, v); v = dpp64b<0x114, 0x2>(v, v); v = dpp64b<0x118, 0xc>(v, v);
        return v;
    }
    // v from the next lane of the group; the last lane gets `fill`
    __device__ static __forceinline__ double next_or(double fill, double v, int) { return dppv<0x101, 0xf, false>(fill, v); }
};
// LPI = 32: two rows per group (two instances per wavefront; R = 4 samples per lane at N <= 128).  Row-local DPP steps as for
// 16, one exchange with the partner row (lane ^ 16: ds_swizzle) for the sums, readlane of lanes 16 / 48 for the scan's fifth step.
__device__ __forceinline__ double swz16(double v)       // the value of lane ^ 16
{
    return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), 0x401F), __builtin_amdgcn_ds_swizzle(__double2loint(v), 0x401F));
}
template <> struct Grp<32> {
    static constexpr int STEPS = 5;
    __device__ static __forceinline__ double sum(double v)
    {
        v += dpp64n<0x121, false>(v); v += dpp64n<0x122, false>(v); v += dpp64n<0x124, false>(v); v += dpp64n<0x128, false>(v);
        return v + swz16(v);
    }
    __device__ static __forceinline__ int sum_i(int v)
    {
        v += __builtin_amdgcn_mov_dpp(v, 0x121, 0xf, 0xf, false); v += __builtin_amdgcn_mov_dpp(v, 0x122, 0xf, 0xf, false);
        v += __builtin_amdgcn_mov_dpp(v, 0x124, 0xf, 0xf, false); v += __builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, false);
        return v + __builtin_amdgcn_ds_swizzle(v, 0x401F);
    }
    // steps 0-3 stay inside a row (v from lane + 2^K of the ROW, 0 past its end); step 4 is grp_scan_step's own
    template <int K> __device__ static __forceinline__ double shl0(double v, int) { return dpp64n<0x100 + (1 << K), true>(v); }
    __device__ static __forceinline__ double bcast0(double v)
    {
        const double a = readlane64<0>(v), b = readlane64<32>(v);
        return ((threadIdx.x & 32) != 0) ? b : a;
    }
    // v from the next lane of the group (wave_shl:1 crosses the row boundary); the last lane gets `fill`
    __device__ static __forceinline__ double next_or(double fill, double v, int li)
    {
        const double t = dppv<0x130, 0xf, false>(fill, v);
        return (li == 31) ? fill : t;
    }
};
template <> struct Grp<8> {
    static constexpr int STEPS = 3;
    __device__ static __forceinline__ double sum(double v)
    {
        v += dpp64n<0x0B1, false>(v);                                  // quad_perm [1,0,3,2]
        v += dpp64n<0x04E, false>(v);                                  // quad_perm [2,3,0,1]
        v += dpp64n<0x141, false>(v);                                  // row_half_mirror: lane l <-> 7 - l of its half row
        return v;
    }
    __device__ static __forceinline__ int sum_i(int v)
    {
        v += __builtin_amdgcn_mov_dpp(v, 0x0B1, 0xf, 0xf, false); v += __builtin_amdgcn_mov_dpp(v, 0x04E, 0xf, 0xf, false);
        v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, false);
        return v;
    }
    template <int K> __device__ static __forceinline__ double shl0(double v, int li)
    {
        if constexpr (K == 2) return dpp64b<0x104, 0x5>(0.0, v);      // banks 0 and 2 read lanes + 4; banks 1 and 3 stay 0
        else { const double t = dpp64n<0x100 + (1 << K), true>(v); return (li + (1 << K) < 8) ? t : 0.0; }
    }
    __device__ static __forceinline__ double bcast0(double v)
    {
        v = dpp64b<0x000, 0xf>(v, v); v = dpp64b<0x114, 0xa>(v, v);    // quad_perm [0,0,0,0]; banks 1,3 <- banks 0,2
        return v;
    }
    __device__ static __forceinline__ double next_or(double fill, double v, int li)
    {
        const double t = dppv<0x101, 0xf, false>(fill, v);
        return (li == 7) ? fill : t;
    }
};
// y <- T y for T = I + Tm taken from lane + 2^K of the group (Tm = 0 past the end of the group)
template <int LPI, int K>
__device__ __forceinline__ void grp_scan_step(M2& y, int li)
{
    if constexpr (LPI == 32 && K == 4) {
        // the rows have their own suffix products; the lower row of a group still needs the upper row's total (its lane 16 / 48)
        const bool g1 = (threadIdx.x & 32) != 0, low = li < 16;
        const double ya = g1 ? readlane64<48>(y.a) : readlane64<16>(y.a), yb = g1 ? readlane64<48>(y.b) : readlane64<16>(y.b);
        const double yc = g1 ? readlane64<48>(y.c) : readlane64<16>(y.c), yd = g1 ? readlane64<48>(y.d) : readlane64<16>(y.d);
        const double ta = low ? ya - 1.0 : 0.0, tb = low ? yb : 0.0, tc = low ? yc : 0.0, td = low ? yd - 1.0 : 0.0;
        M2 r;
        r.a = fma(ta, y.a, fma(tb, y.c, y.a)); r.b = fma(ta, y.b, fma(tb, y.d, y.b));
        r.c = fma(tc, y.a, fma(td, y.c, y.c)); r.d = fma(tc, y.b, fma(td, y.d, y.d));
        y = r;
    } else
    if constexpr (K < Grp<LPI>::STEPS) {
        const double ta = Grp<LPI>::template shl0<K>(y.a - 1.0, li), tb = Grp<LPI>::template shl0<K>(y.b, li);
        const double tc = Grp<LPI>::template shl0<K>(y.c, li), td = Grp<LPI>::template shl0<K>(y.d - 1.0, li);
        M2 r;
        r.a = fma(ta, y.a, fma(tb, y.c, y.a)); r.b = fma(ta, y.b, fma(tb, y.d, y.b));
        r.c = fma(tc, y.a, fma(td, y.c, y.c)); r.d = fma(tc, y.b, fma(td, y.d, y.d));
        y = r;
    }
}

// One tick of one instance per lane group, registers in, registers out.  `s.w` is the WalkState the tick runs with (caller
// bookkeeping already applied).  Returns true in every lane of a group whose instance has active vertical inequality rows
// (deferred to the active-set fallback; its QOut is then provisional).
// LDS of one wavefront of the lane-group kernels: the midpoint window of each of its instances, staged so that the global
// loads are coalesced (lane li reads sample k LPI + li) and every lane then picks up its own R consecutive samples.  A lane's
// block starts at li * MIDM double2; MIDM is odd, which keeps the 16-byte reads of 16 lanes on 16 different bank quads.
template <int R> constexpr int midm() { return R | 1; }
template <int R, int LPI> constexpr int wave_lds_double2() { return (64 / LPI) * LPI * midm<R>(); }
// ... and, in the kernels that run the inequality fallback themselves, at least the fallback's working window (z_active_set)
template <int R, int LPI> constexpr int wave_lds_double2_fb() { return wave_lds_double2<R, LPI>() > (Z_LDS_DOUBLES + 1) / 2 ? wave_lds_double2<R, LPI>() : (Z_LDS_DOUBLES + 1) / 2; }

// Tried and dropped for the knapsack loop: count and sums of both axes in one pass (six interleaved reductions) -- slower on MI355X
// at every size: 10.2 vs 9.7 us at 1 024 instances, 14.0 vs 12.8 at 8 192, 51.8 vs 46.7 at 65 536, 5.9 vs 5.4 per rollout tick.
// SW: parameter sweep -- the groups of a wavefront may belong to different parameter sets: what depends on the set (tables
// of the vertical stage, tails, mass, eta, box widths, bounds on S u) is read through the instance's own record c.sets[s.ps]
// (per-lane loads); horizon, plan, dt, g and the gate are the handle's.  SW = 0 compiles to exactly the plain kernel.
// SW = 2: multi-plan handle -- the record is the one of the instance's (set, plan) pair, and the plan is read through it too: the
// midpoint window (the same coalesced load from another base address), the tails and, in the callers, the step timings.
// `keep` (group-uniform): will anything of this group be stored?  A tail group, whose record nobody reads, never enters the knapsack
// loop.  MF: a group in flight or gated does not enter it either.  That is the per-tick kernels; the rollout passes MF = false,
// which masks nothing (keep is not read) and compiles to the loop it always had: it sets one simulation time for its whole batch, so its
// wavefronts hold one gait phase, and both a flight test and a parking mask (valid && alive) measured slower there
// (scripts/bench_rollout.py, -1 to -3 %).
// Horizon padding (LPI R slots for N samples; at N = 100, R = 13 only lane 7 owns padded ones, but every slot of every lane paid for the masks):
// harmless by data wherever that changes no bit -- the bound check on S u without a mask when zlo <= 0 <= zhi in the whole wavefront (a padded
// su is exactly 0), the midpoint sums without selects (a padded a_n is exactly +-0), the midpoint window without a clamp (zero slack behind the
// tables), r < N - n0 where a mask stays, and gate_tick's remainder and division behind uniform branches.  Records, u_traj and rollouts hash equal
// to the parent's on every case of DESIGN section 5.  Measured, one box, builds alternated round-robin, five runs each, 65 536 instances
// (10^9 ticks/s | isolated kernel us): parent 1.560-1.595 | 43.7-46.2 (one run 41.0); this 1.603-1.658 | 42.8-43.0 (one 39.7).  Each cut alone
// against the parent is inside the parent's spread (bound check 1.547-1.596, midpoints 1.591-1.615, clamp 1.573-1.600, gate 1.564-1.591); what
// decided is the set with one cut left out against the whole set (1.619-1.666 | 42.4-42.9): without the bound check 1.586-1.611 | 43.4-44.3,
// without the midpoint cut 1.583-1.650 | 43.3-44.2, without the clamp cut 1.577-1.631 | 42.6-43.0, without the gate's 1.593-1.631 | 43.1-43.6.
// Dropped: dt_n of a slot from a per-layout table instead of the select (a new table, upload and DevConst field; -26 selects, +13 loads per
// lane): the whole set above is WITH it, this build without -- a tie on both figures, so the select stays.
template <int R, int LPI, int SW = 0, bool MF = true, bool MASKS = MF>
__device__ __forceinline__ bool tick_group_core(const DevConst& c, const int lane, const QState& s, QOut& o, double* __restrict__ u_traj_inst,
                                                double2* __restrict__ lds_wave, const bool keep)
{
    constexpr int NT = ismpc::Tables::NT;
    const int N = c.N;
    const int li = lane & (LPI - 1);                  // lane inside the group = inside the instance
    const double dt = c.dt;
    const Walk& w = s.w;
    const double x0 = s.x, y0 = s.y, z0 = s.z, xd0 = s.xd, yd0 = s.yd, zd0 = s.zd;
    const DevConst* P = SW ? c.sets + (s.ps >= 0 ? s.ps : 0) : nullptr;
    const double* p_vqT = SW ? P->vqT : c.vqT;
    const double p_z_lo = SW ? P->z_lo : c.z_lo, p_z_hi = SW ? P->z_hi : c.z_hi;
    const double p_inv_mass = SW ? P->inv_mass : c.inv_mass, p_inv_eta = SW ? P->inv_eta : c.inv_eta;
    const double p_half_run = SW ? P->half_run : c.half_run, p_half_first = SW ? P->half_first : c.half_first;
    const double* p_tailx = SW ? P->tailx : c.tailx; const double* p_taily = SW ? P->taily : c.taily;
    const double p_dt_over_mass = SW ? P->dt_over_mass : c.dt_over_mass, p_h_des = SW ? P->h_des : c.h_des;
    const double* p_midxy = SW == 2 ? P->midxy : c.midxy;
    int idx;
    const int gate_status = gate_tick<MF>(c, w, idx) | ((SW && s.ps < 0) ? ISMPC_ST_BAD_INDEX : 0);     // group-uniform; a gated group runs the arithmetic on idx = 0 and drops it
    int status = gate_status;
    const bool run = gate_status == 0;
    if (!run) idx = 0;
    const int n0 = li * R;                            // this lane owns samples n0 .. n0+R-1 (tables are zero past N)
    const int nv = N - n0;                            // ... of which slots r < nv are samples of the horizon (the others are padding)
    // MF = false (the rollout) keeps every mask, the clamp and the compares as they were: with them gone scripts/bench_rollout.py lost 1.6 % at
    // 65 536 instances without a trajectory (1.731-1.736 -> 1.701-1.708e9 ticks/s, three alternations), and that kernel is kept only if it does not lose
    constexpr bool LEAN = MF;
    auto in_horizon = [&](int r) { return LEAN ? r < nv : n0 + r < N; };
    STAMP_DECL;
    STAMP(1);                                         // the record has arrived (gate_tick consumed it)

    // ---- vertical stage from the affine tables (MPCSolver.cpp:223-243, is_running :262-263)
    const int pat = (run && w.fc > 1 && w.mpc < c.npat) ? w.mpc : c.npat;
    const double2* T = reinterpret_cast<const double2*>(p_vqT) + (size_t)pat * (R * 3 * LPI) + li;  // 3 x 16 bytes per sample, lane-contiguous
    // midpoint window [idx, idx + LPI R) of this instance -> LDS, coalesced (consumed after the scan; MPCSolver.cpp:328-338,388-389)
    constexpr int MIDM = midm<R>();
    double2* Lm = lds_wave + (lane / LPI) * (LPI * MIDM);
    // No clamp at the end of the table: the gate admits idx + 2 N <= nmid and the window reads up to idx + LPI R - 1 <= nmid - 2 N + 127, which
    // every midxy allocation covers with MIDXY_SLACK zero entries behind its last plan (ismpc_hip.hip).  Inside a multi-plan slab the read runs
    // into the next plan's midpoints instead: finite values in padded slots, which the sums below multiply by an exact zero.
    const double2* Mw = reinterpret_cast<const double2*>(p_midxy) + (unsigned)(idx + li);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int j = k * LPI + li;
        if constexpr (LEAN) Lm[(j / R) * MIDM + (j % R)] = Mw[k * LPI];
        else Lm[(j / R) * MIDM + (j % R)] = reinterpret_cast<const double2*>(p_midxy)[min(idx + j, c.nmid - 1)];
    }
    double u[R], su[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double2 t01 = T[(3 * r) * LPI], t23 = T[(3 * r + 1) * LPI], t45 = T[(3 * r + 2) * LPI];
        u[r] = fma(zd0, t23.x, fma(z0, t01.y, t01.x));
        su[r] = fma(zd0, t45.y, fma(z0, t45.x, t23.y));
    }
    // Extrema of S u against the bounds.  A padded slot has su = 0 exactly (its table entries are zero; a non-finite state makes it NaN, which
    // fmin / fmax pass over), so the extrema over ALL R slots are min(smin, 0) and max(smax, 0): `viol` below is the same decision whenever
    // zlo_t <= 0 <= zhi_t.  That is tested once per wavefront (the bounds are per instance in a sweep); a wavefront with a bound on the other
    // side of zero -- or a NaN one -- takes the masked loop.
    const double zlo_t = p_z_lo - z_tol(p_z_lo), zhi_t = p_z_hi + z_tol(p_z_hi);
    double smin = INFINITY, smax = -INFINITY;
    if (LEAN && __builtin_amdgcn_ballot_w64(!(zlo_t <= 0.0 && zhi_t >= 0.0)) == 0ull) {
#pragma unroll
        for (int r = 0; r < R; ++r) { smin = fmin(smin, su[r]); smax = fmax(smax, su[r]); }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (in_horizon(r)) { smin = fmin(smin, su[r]); smax = fmax(smax, su[r]); }
    }
    if (!c.flat) {                                      // plans with mid_z != 0 (MPCSolver.cpp:259): per-frame offsets, pattern corrections
        int elo = 0, ne = 0;
        if (pat < c.npat) { elo = c.e_lo[pat]; ne = c.ne[pat]; }
        const int pp = pat < c.npat ? pat : 0;
        int nemax = 0;
#pragma unroll
        for (int g = 0; g < 64; g += LPI) nemax = max(nemax, __builtin_amdgcn_readlane(ne, g));
        const double* dUr = (SW ? P->dU : c.dU) + (size_t)idx * NT;          // (a sweep: this instance's set has its own offsets and corrections)
        const double* sUr = (SW ? P->SdU : c.SdU) + (size_t)idx * NT;
        double du[R], ds[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { du[r] = dUr[n0 + r]; ds[r] = sUr[n0 + r]; }
        for (int e = 0; e < nemax; ++e) {
            const bool on = e < ne;
            const double ue = on ? dUr[elo + e] : 0.0;
            const double* wr = (SW ? P->Wt : c.Wt) + ((size_t)pp * c.Fmax + (on ? e : 0)) * NT + n0;
            const double* sr = (SW ? P->SW : c.SW) + ((size_t)pp * c.Fmax + (on ? e : 0)) * NT + n0;
#pragma unroll
            for (int r = 0; r < R; ++r) { du[r] = fma(-wr[r], ue, du[r]); ds[r] = fma(-sr[r], ue, ds[r]); }
        }
        smin = INFINITY; smax = -INFINITY;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = n0 + r;
            u[r] += du[r]; su[r] += ds[r];
            if (n >= elo && n < elo + ne) u[r] = 0.0;
            if (in_horizon(r)) { smin = fmin(smin, su[r]); smax = fmax(smax, su[r]); }      // (masked: no bench leg runs a plan with heights)
        }
    }
    const bool viol = smin < zlo_t || smax > zhi_t;                                                // MPCSolver.cpp:158-160, beyond rounding
    const unsigned long long vmask = __builtin_amdgcn_ballot_w64(viol);
    const bool deferred = run && (((vmask >> (lane & (64 - LPI))) & ((1ull << LPI) - 1ull)) != 0ull);
    if (deferred) status |= ISMPC_ST_Z_INEQ_ACTIVE;

    // ---- lambda_j (MPCSolver.cpp:306) and A_j, B_j (:353-361): A = [1+wQ, dt P; lam dt P, 1+wQ], B = [-wQ, -lam dt P]
    double ch1[R], s1[R], s2[R], lam0_l = 0.0;
    bool big = false, mid = false;
    {
        double wv_[R], le_[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double2 tq = reinterpret_cast<const double2*>(c.tzgT)[r * LPI + li];
            const double zpos = su[r] + fma(tq.x, zd0, z0) + tq.y;                  // S u + T_bar_z s + T_bar_g_z
            const double zacc = fma(p_inv_mass, u[r], -c.g);
            const double lam = (c.g + zacc) * frcp(zpos);
            if (r == 0) lam0_l = lam;
            le_[r] = (lam < c.gate) ? 0.0 : lam;
            const double dtn = in_horizon(r) ? dt : 0.0;
            wv_[r] = le_[r] * dtn * dtn;
            s1[r] = dtn;                                  // dt_n for now
            big = big || (wv_[r] > 0.25);
            mid = mid || (wv_[r] > 0.004);
        }
        if (__builtin_amdgcn_ballot_w64(mid) == 0) {      // degree 3 (taylor_low) in every group of the wavefront
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double P = TAYLOR_P3, Q = TAYLOR_Q3;
                taylor_low(wv_[r], P, Q);
                ab_series(wv_[r], s1[r], le_[r], P, Q, ch1[r], s1[r], s2[r]);
            }
        } else {
            // some group of this wavefront needs the long polynomial.  The choice is made PER GROUP (= per instance): a group whose own
            // samples all have w <= 0.004 takes the degree-3 values here too, so an instance's record does not depend on which instances
            // share its wavefront (round 4: a sweep sorted by parameter set, ismpc_sweep_bind, changes an instance's wave-mates)
            const bool gmid = ((__builtin_amdgcn_ballot_w64(mid) >> (lane & (64 - LPI))) & ((LPI == 64) ? ~0ull : ((1ull << LPI) - 1ull))) != 0ull;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double dtn = s1[r];
                double P, Q;
                taylor_high(wv_[r], P, Q);
                P = gmid ? P : TAYLOR_P3;   Q = gmid ? Q : TAYLOR_Q3;   // (degree 3 starts here)
                taylor_low(wv_[r], P, Q);
                ab_series(wv_[r], dtn, le_[r], P, Q, ch1[r], s1[r], s2[r]);
                if (__builtin_amdgcn_ballot_w64(big) != 0 && wv_[r] > 0.25) ab_libm(wv_[r], dtn, le_[r], ch1[r], s1[r], s2[r]);     // lambda dt^2 > 1/4: off any physical gait
            }
        }
    }
    // ---- inclusive suffix product over the group: Y_l = A(block LPI-1) ... A(block l); C_sc = [1, 1/eta]
    M2 Y = (M2){1.0 + ch1[0], s1[0], s2[0], 1.0 + ch1[0]};
#pragma unroll
    for (int r = 1; r < R; ++r) Y = mul((M2){1.0 + ch1[r], s1[r], s2[r], 1.0 + ch1[r]}, Y);
    STAMP(2);                                         // tables arrived, lambda / A_j / local products done
    grp_scan_step<LPI, 0>(Y, li); grp_scan_step<LPI, 1>(Y, li); grp_scan_step<LPI, 2>(Y, li); grp_scan_step<LPI, 3>(Y, li);
    grp_scan_step<LPI, 4>(Y, li);
    const double ie = p_inv_eta;
    const double cva = fma(ie, Y.c, Y.a), cvb = fma(ie, Y.d, Y.b);       // C_sc (suffix product from this lane's first sample)
    double c0 = Grp<LPI>::next_or(1.0, cva, li), c1 = Grp<LPI>::next_or(ie, cvb, li);                 // the lane needs it one lane up
    // ---- Aeq(n) = C_sc phi_input(:,n) = c_n B_n, walking the lane's samples backwards
    double a[R];
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
        a[r] = -fma(c0, ch1[r], c1 * s2[r]);
        const double k0 = fma(c0, ch1[r], fma(c1, s2[r], c0)), k1 = fma(c1, ch1[r], fma(c0, s1[r], c1));
        c0 = k0; c1 = k1;
    }
    const double h = (w.fc > 1) ? p_half_run : p_half_first;                                          // MPCSolver.cpp:328-338
    double q0 = 0.0, s_ax = 0.0, s_ay = 0.0, mx0 = 0.0, my0 = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();          // the staged window is complete
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // No mask on a padded slot: its a[r] is +-0 exactly (ch1 = s2 = 0 where dt_n = 0) and what the window holds there is finite (the
        // plan's later midpoints, the next plan's, or the zero slack), so fma(+-0, m, s) = s -- s starts at +0 and a sum that is never -0
        // stays what it was.  Where a[r] is NaN (a non-finite state) the masked form fma(NaN, 0, s) was NaN just as well.
        const double2 mq = Lm[li * MIDM + r];
        const double mx = (LEAN || in_horizon(r)) ? mq.x : 0.0, my = (LEAN || in_horizon(r)) ? mq.y : 0.0;
        if (r == 0) { mx0 = mx; my0 = my; }               // (read in lane 0 only, whose first sample is inside every horizon)
        q0 = fma(a[r], a[r], q0); s_ax = fma(a[r], mx, s_ax); s_ay = fma(a[r], my, s_ay);
    }
    q0 = Grp<LPI>::sum(q0); s_ax = Grp<LPI>::sum(s_ax); s_ay = Grp<LPI>::sum(s_ay);
    // C_sc phi_state sits in lane 0 of the group (cva, cvb there); beq - a'mid (MPCSolver.cpp:381-384), group-uniform
    const double bpx = Grp<LPI>::bcast0((p_tailx[idx] - fma(cva, x0, cvb * xd0)) - s_ax);
    const double bpy = Grp<LPI>::bcast0((p_taily[idx] - fma(cva, y0, cvb * yd0)) - s_ay);
    const double sgx = (bpx < 0.0) ? -1.0 : 1.0, sgy = (bpy < 0.0) ? -1.0 : 1.0;
    STAMP(3);                                         // scan, backward walk, midpoints, reductions done
    // min 1/2|v|^2, a'v = bp, |v| <= h  ->  v_n = sg sign(a_n) min(tau |a_n|, h): Newton on the concave piecewise-linear
    // G(tau) = sum |a_n| min(tau |a_n|, h) from tau = 0; the groups iterate in lockstep, each with its own state
    const double Tq[2] = { fabs(bpx), fabs(bpy) };
    const double iq0 = frcp(q0);
    double tau[2] = { Tq[0] * iq0, Tq[1] * iq0 };
    int its[2] = {1, 1}, prev[2] = {0, 0};
    // Nothing of stage 3 survives for a group in flight (lam0 <= gate, MPCSolver.cpp:322; a NaN lam0 is flight, as in the integration
    // below) or a gated one: ux0, uy0, itx, ity stay 0, st3 is not merged, the u_traj rows of x and y are 0.  Such a group is never
    // live, so it does not keep the other groups of its wavefront in the loop.  (A deferred group stays live: its provisional record
    // is observable in the two-launch form and with ISMPC_Z_FALLBACK=0.)  A group that is not live keeps tau at its start; its
    // ux0 / uy0 are then not the converged ones, and none of it is stored (every store of a tail group is guarded by `valid`).
    const bool stage3 = run && Grp<LPI>::bcast0(lam0_l) > c.gate;
    int st3 = 0;
    if (!(q0 > 0.0)) {                                                       // no sample can move the ZMP
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) {
            tau[ax] = (Tq[ax] > 0.0) ? INFINITY : 0.0;
            if (Tq[ax] > 1e-300) st3 |= (ax == 0 ? ISMPC_ST_X_INFEASIBLE : ISMPC_ST_Y_INFEASIBLE);
        }
    }
    // MASKS (the per-tick kernels, tied to MF as LEAN is): which groups are live is kept in two wave-wide 64-bit lane masks, one per axis, in
    // scalar registers.  As per-lane bools the two flags sat packed in one VGPR and every "is anyone live" test was a round trip mask -> VGPR ->
    // mask (v_and_b32_sdwa, v_cmp_eq_u32, v_cndmask 0/1, v_cmp_ne_u32), the update below a three-deep exec nest with copies of tau.  Here the
    // tests are s_cmp on the mask, a mask is only ever written from a ballot at a point every lane reaches (never inside divergent code), and a
    // lane reads its flag back with the inverse ballot of that wave-uniform value.
    // Every QP sees the iterate sequence it saw: a lane's bit of lv[ax] is the live[ax] it had at the same point of the same pass.
    //   - cnt == prev clears the bit exactly where `live && cnt == prev` cleared the flag (and-not of a ballot taken in all lanes).
    //   - rem, tn and the three compares are computed in every lane from the group's sums; only a live lane stores anything of them.  A live lane
    //     stores ++its; with allsat = !(qfree > 0) (true for qfree = 0 and for NaN) tau = INFINITY and the infeasible bit under the same test
    //     as before, and the bit goes; otherwise tn = rem * frcp(qfree) and grow = tn > tau (false for a NaN tn): tau = tn and prev = cnt if it
    //     grows, nothing but the cleared bit if not.  Those are the three branches the loop had, as selects.  q0 <= 0 is settled before the loop
    //     as it was: such a group enters live with tau = INFINITY or 0, counts, and leaves through cnt == prev or through allsat exactly as before.
    //   - A lane that is not live computes garbage (frcp of 0 included: rcp and fma raise nothing on this path) and stores none of it; every
    //     outcome mask is and-ed with the live mask.
    //   - One ballot per compare, combined with s_and / s_andn2: a ballot of `a && b` comes back through v_cndmask 0/1 + v_cmp_ne.
    // Measured (the record is DESIGN section 5), parent's library against this one, alternated: SQ_INSTS_VALU / SQ_WAVES of the headline
    // 1 714.97 -> 1 654.13, 65 536 instances 1.606-1.628 -> 1.668-1.709 10^9 ticks/s (every run above every run of the parent), isolated launch
    // 39.7-42.7 -> 37.9-40.8 us.  The sum pass under the exec mask, tried on top, was slower (46.1-47.6 us) and is not here.
    // The rollout (MF = false) keeps the loop it had, verbatim: with the masks one of its instantiations does not compile (the backend's verifier
    // on the null test of the LDS window, as in the disturbed rollout) and several of those that do gain spilled vector registers.
    if constexpr (MASKS) {
        const unsigned long long lv0 = __builtin_amdgcn_ballot_w64(MF ? keep && stage3 : true);
        unsigned long long lv[2] = {lv0, lv0};
        for (int it = 0; it < N + 2; ++it) {
            if ((lv[0] | lv[1]) == 0ull) break;
#pragma unroll
            for (int ax = 0; ax < 2; ++ax) {
                if (lv[ax] == 0ull) continue;                                 // this axis is done in every group of the wavefront (the other one
                                                                              // may keep the loop alive: scripts/knapsack_model.py)
                int cl = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) cl += (tau[ax] * fabs(a[r]) >= h) ? 1 : 0;
                const int cnt = Grp<LPI>::sum_i(cl);
                lv[ax] &= ~__builtin_amdgcn_ballot_w64(cnt == prev[ax]);      // active set unchanged: exact
                if (lv[ax] == 0ull) continue;
                double ssat = 0.0, qfree = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // 0 / 1 masks and two fused multiply-adds instead of two 64-bit selects and two adds: the same sums bit for bit
                    // (fma(1, x, s) = s + x rounded once, fma(0, x, s) = s), a third fewer instructions in the loop the kernel spends most in
                    const double ab = fabs(a[r]);
                    const bool sat = tau[ax] * ab >= h;
                    const double ms = sat ? 1.0 : 0.0, mf = sat ? 0.0 : 1.0;
                    ssat = fma(ms, ab, ssat); qfree = fma(mf, a[r] * a[r], qfree);
                }
                ssat = Grp<LPI>::sum(ssat); qfree = Grp<LPI>::sum(qfree);
                const double rem = fma(-h, ssat, Tq[ax]);
                const double tn = rem * frcp(qfree);
                // the outcomes as lane masks of the live lanes (one ballot per compare, combined on the scalar unit); each store is one
                // select under the inverse ballot of its mask.  allsat = !(qfree > 0): everything saturated; grow = !allsat && tn > tau
                const unsigned long long m_live = lv[ax];
                const unsigned long long b_free = __builtin_amdgcn_ballot_w64(qfree > 0.0);
                const unsigned long long m_grow = m_live & b_free & __builtin_amdgcn_ballot_w64(tn > tau[ax]);
                const unsigned long long m_sat = m_live & ~b_free;
                const unsigned long long m_inf = m_sat & __builtin_amdgcn_ballot_w64(rem > fma(h * ssat, 1e-12, 1e-300));
                its[ax] += __builtin_amdgcn_inverse_ballot_w64(m_live) ? 1 : 0;
                st3 |= __builtin_amdgcn_inverse_ballot_w64(m_inf) ? (ax == 0 ? ISMPC_ST_X_INFEASIBLE : ISMPC_ST_Y_INFEASIBLE) : 0;
                tau[ax] = __builtin_amdgcn_inverse_ballot_w64(m_sat) ? INFINITY : __builtin_amdgcn_inverse_ballot_w64(m_grow) ? tn : tau[ax];
                prev[ax] = __builtin_amdgcn_inverse_ballot_w64(m_grow) ? cnt : prev[ax];
                lv[ax] = m_grow;
            }
        }
    } else {
    bool live[2] = {true, true};
    for (int it = 0; it < N + 2; ++it) {
        if (__builtin_amdgcn_ballot_w64(live[0] || live[1]) == 0ull) break;
#pragma unroll
        for (int ax = 0; ax < 2; ++ax) {
            if (__builtin_amdgcn_ballot_w64(live[ax]) == 0ull) continue;      // this axis is done in every group of the wavefront (the other one
                                                                              // may keep the loop alive: scripts/knapsack_model.py)
            int cl = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) cl += (tau[ax] * fabs(a[r]) >= h) ? 1 : 0;
            const int cnt = Grp<LPI>::sum_i(cl);
            if (live[ax] && cnt == prev[ax]) live[ax] = false;                // active set unchanged: exact
            if (__builtin_amdgcn_ballot_w64(live[ax]) == 0ull) continue;
            double ssat = 0.0, qfree = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                // 0 / 1 masks and two fused multiply-adds instead of two 64-bit selects and two adds: the same sums bit for bit
                // (fma(1, x, s) = s + x rounded once, fma(0, x, s) = s), a third fewer instructions in the loop the kernel spends most in
                const double ab = fabs(a[r]);
                const bool sat = tau[ax] * ab >= h;
                const double ms = sat ? 1.0 : 0.0, mf = sat ? 0.0 : 1.0;
                ssat = fma(ms, ab, ssat); qfree = fma(mf, a[r] * a[r], qfree);
            }
            ssat = Grp<LPI>::sum(ssat); qfree = Grp<LPI>::sum(qfree);
            if (live[ax]) {
                ++its[ax];
                const double rem = fma(-h, ssat, Tq[ax]);
                if (!(qfree > 0.0)) {                                         // everything saturated
                    if (rem > fma(h * ssat, 1e-12, 1e-300)) st3 |= (ax == 0 ? ISMPC_ST_X_INFEASIBLE : ISMPC_ST_Y_INFEASIBLE);
                    tau[ax] = INFINITY; live[ax] = false;
                } else {
                    const double tn = rem * frcp(qfree);
                    if (!(tn > tau[ax])) live[ax] = false;
                    else { tau[ax] = tn; prev[ax] = cnt; }
                }
            }
        }
    }
    }

    STAMP(4);                                         // knapsack Newton done
    // ---- lane 0 of the group finishes the instance: integration (MPCSolver.cpp:274-278, 406-422)
    o.x = x0; o.y = y0; o.z = z0; o.xd = xd0; o.yd = yd0; o.zd = zd0;
    o.uz0 = 0.0; o.ux0 = 0.0; o.uy0 = 0.0; o.itx = 0; o.ity = 0;
    if (li == 0 && run) {
        o.uz0 = u[0];
        integrate_z(c, p_dt_over_mass, p_h_des, z0, zd0, o.uz0, o.z, o.zd, status);
        const double A0a = 1.0 + ch1[0], A0b = s1[0], A0c = s2[0];
        if (lam0_l > c.gate) {                                            // MPCSolver.cpp:322
            status |= st3; o.itx = its[0]; o.ity = its[1];
            o.ux0 = box_move(sgx, a[0], tau[0], h, mx0);
            o.uy0 = box_move(sgy, a[0], tau[1], h, my0);
        } else status |= ISMPC_ST_FLIGHT;
        integrate_xy(A0a, A0b, A0c, x0, xd0, o.ux0, o.x, o.xd);
        integrate_xy(A0a, A0b, A0c, y0, yd0, o.uy0, o.y, o.yd);
    }
    o.status = status;
    if (u_traj_inst) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = n0 + r;
            if (in_horizon(r)) {
                double vx = 0.0, vy = 0.0;
                if (stage3) {
                    // (SW = 2: the plan's midpoints from the staged window -- the same values, and the pair's record need not stay live)
                    const double2 mq = SW == 2 ? Lm[li * MIDM + r] : make_double2(c.midx[idx + n], c.midy[idx + n]);
                    vx = box_move(sgx, a[r], tau[0], h, mq.x);
                    vy = box_move(sgy, a[r], tau[1], h, mq.y);
                }
                u_traj_inst[n] = run ? u[r] : 0.0; u_traj_inst[N + n] = vx; u_traj_inst[2 * N + n] = vy;
            }
        }
    }
    return deferred;
}

// One launch = one tick: record in, record out (and, in the host-driven closed loop, state fed back in place)
template <int R, int LPI, int SW = 0>
__device__ __forceinline__ bool tick_group_body(const DevConst& c, const int gi_raw, const int batch, const int lane,
                                                const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                                                ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj,
                                                int rollout_frame, unsigned char* zmark, int launch_id, double2* __restrict__ lds_wave, int* zlist = nullptr)
{
    const bool valid = gi_raw < batch;
    const int gi = valid ? gi_raw : batch - 1;        // tail groups recompute the last instance and store nothing
    STAMP_DECL;
    STAMP(0);                                         // first instructions of the wavefront
    const ismpc_tick_in* rec = ((rollout_frame >= 0) ? state_rw : in_ro) + gi;
    QState s;
    // s.ps: the instance's record (-1, an unknown set or pair: ISMPC_ST_BAD_INDEX, state passed through).  A multi-plan
    // handle needs it first: the caller bookkeeping runs on ITS plan's step timings.  Otherwise it is read last: read
    // first it costs ismpc_tick_quad_one<13, 8, 2, 1> four spilled VGPRs and 32 bytes of scratch
    if constexpr (SW == 2) s.ps = record_index<SW>(c, rec->reserved);
    s.w = load_walk(c, SW == 2 ? c.sets[max(s.ps, 0)].ftsp_t : c.ftsp_t, rec, rollout_frame);
    load_com(rec, s);
    if constexpr (SW != 2) s.ps = SW ? record_index<SW>(c, rec->reserved) : 0;
    QOut o;
    const bool deferred = tick_group_core<R, LPI, SW>(c, lane, s, o, (u_traj && valid) ? u_traj + (size_t)gi * 3 * c.N : nullptr, lds_wave, valid);
    if ((lane & (LPI - 1)) == 0 && valid) {
        if (out) store_record(out + gi, o);
        if (deferred) {
            if (c.zseen) *c.zseen = launch_id;
            if (zlist) { const int slot = atomicAdd(c.zflag, 1); if (slot < batch) zlist[slot] = gi; }
        }
        if (rollout_frame >= 0 && !deferred) store_feedback(c, state_rw + gi, o, s.w);
    }
    STAMP(5);                                         // stores issued
    STAMP_WHERE;
    return deferred && valid;
}

#ifndef ISMPC_QUAD_WAVES
#define ISMPC_QUAD_WAVES 4
#endif
// Workgroups are handed to the 8 XCDs round-robin (workgroup b runs on XCD b mod 8, each with its own L2).  The virtual block of
// workgroup b: XCD x takes the contiguous range [x q + min(x, r), ...) of the nb blocks (q = nb / 8, r = nb mod 8) -- a bijection.
__device__ __forceinline__ int sweep_vblock(int b, int nb)
{
    const int q = nb >> 3, r = nb & 7, x = b & 7;
    return x * q + min(x, r) + (b >> 3);
}
// instance of launch slot `slot` (see DevConst::order); slots past the batch name no instance
template <int SW> __device__ __forceinline__ int slot_instance(const DevConst& c, int slot, int batch)
{
    if (SW) { if (c.order) return slot < batch ? c.order[slot] : batch; }
    return slot;
}
// Front end of the per-tick kernels: where this wavefront stands -- its lane, its index in the workgroup and in the launch (through the
// virtual block where a sweep is bound).  The wavefront holds the launch slots wave * IPW .. + IPW - 1, lane / LPI picks the group's.
struct QuadFront { int lane, wv, wave; };
template <int SW, int WPG> __device__ __forceinline__ QuadFront quad_front(const DevConst& c)
{
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int blk = (SW && c.order) ? sweep_vblock(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    return (QuadFront){(int)(threadIdx.x & 63), wv, blk * WPG + wv};
}
// Wavefronts per workgroup of the per-tick lane-group kernels, per shape (RESIDENT: ismpc_tick_quad_inline, whose batch is resident at once;
// otherwise ismpc_tick_quad and ismpc_tick_quad_one); quad_launch() sizes grid and block from the same function.  The rollout, the fallback
// launch, the affine and the dense kernels keep ISMPC_QUAD_WAVES.
// Why it matters: LDS is released when the LAST wavefront of a workgroup ends and a workgroup starts only when all its wave slots are free,
// while wave lifetimes differ (the knapsack loop runs in lockstep over a wavefront's instances: 6.6 us at p10, 10.8 at p90).  At R = 13,
// 8 lanes a workgroup of four holds 53 248 B, so a CU's 160 KB admit three of them where registers admit two: a half-finished workgroup
// holds slots nothing can start in.  Measured, one box, the builds alternated, five runs each (10^9 ticks/s; width 4 | 2 | 1):
//   <13, 8> ismpc_tick_quad_one, 65 536 instances  1.464-1.519 | 1.518-1.557 | 1.560-1.597   (kernel 46.9 | 44.7 | 43.6 us)
//   <13, 8> ismpc_tick_quad_one, 32 768            1.266-1.310 | 1.305-1.316 | 1.312-1.346
//   <13, 8> ismpc_tick_quad (64-set sweep, 65 536) 0.978-1.014 | 1.018-1.030 | 1.034-1.044
//   <13, 8> ismpc_tick_quad_inline, 16 384         1.022-1.049 | 0.987-1.005 | 1.020-1.072   (a tie: stays 4)
//   <7, 16> ismpc_tick_quad_inline, 8 192          0.707-0.728 | 0.719-0.731 | 0.700-0.706   (eight runs at 4 and 2: overlapping, stays 4)
// Slot timeline of the 65 536 launch (scripts/slot_timeline.py), width 4 -> 1: refill gaps 11.9 % -> 5.5 % of the slot time (p50 of a gap
// 1.8 -> 0.76 us), tail 16 % both; SQ_WAVE_CYCLES over slot cycles 0.78 -> 0.85, SQ_INSTS_VALU per wavefront 1 902 both.
// A shape's width moves only where every run of the candidate beat every run of width 4 on that shape's bench leg; R = 8 and 16 at 8
// lanes, R = 8 at 16 lanes, the non-resident 16-lane kernels and the multi-plan instantiations (SW = 2) have no leg and stay 4 (at width 1
// ismpc_tick_quad_one<13, 8, 2, 2> would also move from 255 to 256 VGPRs and from 10 to 8 spilled ones; no other kernel's registers move).
// -DISMPC_WPG_8LANE=n (R = 8, 13, 16 at 8 lanes) and -DISMPC_WPG_16LANE=n (R = 7, 8 at 16 lanes) set all three kernels of those shapes
// for A/B builds (build.build(out=..., flags=...), loaded through ISMPC_LIB; scripts/wg_sweep.sh).
template <int R, int LPI, bool RESIDENT = false, int SW = 0> constexpr int tick_wpg()
{
#ifdef ISMPC_WPG_8LANE
    if (LPI == 8) return ISMPC_WPG_8LANE;
#endif
#ifdef ISMPC_WPG_16LANE
    if (LPI == 16 && R >= 7) return ISMPC_WPG_16LANE;
#endif
    if (LPI == 8 && R == 13 && !RESIDENT && SW != 2) return 1;
    return ISMPC_QUAD_WAVES;
}
template <int R, int LPI, int SW = 0>
__global__ __launch_bounds__(64 * (tick_wpg<R, LPI, false, SW>()))
void ismpc_tick_quad(const DevConst c, const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                     ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj, int batch, int rollout_frame,
                     unsigned char* zmark, int launch_id)
{
    constexpr int IPW = 64 / LPI;                      // instances per wavefront
    __shared__ double2 lds_mid[tick_wpg<R, LPI, false, SW>()][wave_lds_double2<R, LPI>()];
    const QuadFront f = quad_front<SW, tick_wpg<R, LPI, false, SW>()>(c);
    if (f.wave * IPW >= batch) return;
    tick_group_body<R, LPI, SW>(c, slot_instance<SW>(c, f.wave * IPW + f.lane / LPI, batch), batch, f.lane, in_ro, state_rw, out, u_traj, rollout_frame,
                                zmark, launch_id, lds_mid[f.wv], zmark ? zlist_of(zmark, batch) : nullptr);
}

// Latency variant for small batches (every wavefront resident at once): a wavefront that deferred one of its
// instances runs the inequality fallback for it right away, with all 64 lanes, so a step is ONE launch.
template <int R, int LPI, int RW>
__global__ __launch_bounds__(64 * (tick_wpg<R, LPI, true>()), 2)      // two wavefronts per SIMD (that is all a batch that takes this kernel has)
void ismpc_tick_quad_inline(const DevConst c, const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                            ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj, int batch, int rollout_frame,
                            unsigned char* zmark, int launch_id, const DevConst* __restrict__ cdev)
{
    constexpr int IPW = 64 / LPI;
    __shared__ double2 lds_mid[tick_wpg<R, LPI, true>()][wave_lds_double2_fb<R, LPI>()];
    const QuadFront f = quad_front<0, tick_wpg<R, LPI, true>()>(c);
    if (f.wave * IPW >= batch) return;
    const bool def = tick_group_body<R, LPI>(c, f.wave * IPW + f.lane / LPI, batch, f.lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, lds_mid[f.wv]);
    unsigned long long m = __builtin_amdgcn_ballot_w64(def);
    if (m == 0ull) return;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int q = 0; q < IPW; ++q)
        if ((m >> (LPI * q)) & 1ull)
            fallback_call<RW>(cdev, f.wave * IPW + q, f.lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, reinterpret_cast<double*>(lds_mid[f.wv]));   // (the constants in memory:
                                                                                     // taking the address of the by-value argument would move the hot path's copy to the stack)
}

// The one-launch form for batches that do NOT fit the chip at once: the tick keeps the three wavefronts per SIMD of ismpc_tick_quad
// (the kernel asks for them, and the compiler hands that register budget down to the fallback it calls: the fallback spills to
// scratch instead, and only a wavefront that defers an instance runs it).  No second, normally idle, launch per step: +1-2 % at
// 65 536 instances, +4 % at 32 768, +8 % at 16 384 (same box, scripts/ab_env.sh ISMPC_ONE_LAUNCH=0).  SW: parameter sweeps, the
// fallback runs on the deferred instance's own set (SW = 2, multi-plan handles: on the record of its (set, plan) pair).
// wavefronts per SIMD of ismpc_tick_quad<R, LPI, SW> (profiles/r03/kernel_resources.md): what the one-launch form asks for
#ifndef ISMPC_OCC_R13
#define ISMPC_OCC_R13 2
#endif
template <int R, int SW> constexpr int one_occ() { return R <= 4 ? (SW ? 3 : 4) : R <= 7 ? 3 : R == 8 ? (SW ? 2 : 3) : R <= 13 ? ISMPC_OCC_R13 : 1; }
template <int R, int LPI, int RW, int SW>
__global__ __launch_bounds__(64 * (tick_wpg<R, LPI, false, SW>()), (one_occ<R, SW>()))
void ismpc_tick_quad_one(const DevConst c, const ismpc_tick_in* __restrict__ in_ro, ismpc_tick_in* state_rw,
                         ismpc_tick_out* __restrict__ out, double* __restrict__ u_traj, int batch, int rollout_frame,
                         unsigned char* zmark, int launch_id, const DevConst* __restrict__ cdev)
{
    constexpr int IPW = 64 / LPI;
    __shared__ double2 lds_mid[tick_wpg<R, LPI, false, SW>()][wave_lds_double2_fb<R, LPI>()];
    const QuadFront f = quad_front<SW, tick_wpg<R, LPI, false, SW>()>(c);
    if (f.wave * IPW >= batch) return;
    const bool def = tick_group_body<R, LPI, SW>(c, slot_instance<SW>(c, f.wave * IPW + f.lane / LPI, batch), batch, f.lane, in_ro, state_rw, out, u_traj,
                                                 rollout_frame, zmark, launch_id, lds_mid[f.wv]);
    unsigned long long m = __builtin_amdgcn_ballot_w64(def);
    if (m == 0ull) return;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int q = 0; q < IPW; ++q)
        if ((m >> (LPI * q)) & 1ull) {
            const int gi = __builtin_amdgcn_readfirstlane(slot_instance<SW>(c, f.wave * IPW + q, batch));
            const DevConst* cp = cdev;
            if (SW) cp = c.sets + __builtin_amdgcn_readfirstlane(record_index<SW>(c, (((rollout_frame >= 0) ? state_rw : in_ro) + gi)->reserved));   // (a deferred instance has a valid set / pair)
            fallback_call_one<RW, one_occ<R, SW>()>(cp, gi, f.lane, in_ro, state_rw, out, u_traj, rollout_frame, zmark, launch_id, reinterpret_cast<double*>(lds_mid[f.wv]));
        }
}

// Closed loop inside ONE launch (Controller.cpp:297-310 bookkeeping, :346-348 feedback, :503-504 counters): instances are
// independent, so a wavefront keeps the state of its instances in registers for `ticks` ticks and writes one trajectory
// record per tick; nothing but the read-only tables is re-read.  Bit-identical to `ticks` launches of the per-tick kernels
// (same tick_group_core, same fallback body).
//   FB = false (the rollout itself): an instance whose vertical inequality rows become active at tick t parks its pre-tick
//     state in `state`, records t in stop_tick and sits out the rest of the launch;
//   FB = true (second launch, exits at once unless the first one parked something): one wavefront per parked instance
//     resumes it at its tick, running the active-set fallback (all 64 lanes, through memory) at the ticks that need it.
// Keeping the fallback out of the first kernel keeps its register budget that of the tick itself.
//
// MC = true: the disturbed rollout of ismpc_rollout_mc_device -- per-instance velocity pushes in front of a tick, a trajectory
// row every `stride` ticks, one ismpc_rollout_summary per instance.  Everything it adds sits under `if constexpr (MC)`; MC = false
// is the loop above and nothing else.  What lives across tick_group_core (8 lanes, R = 13: 249 VGPRs of 256) stays out of its
// registers: the push cursor, the tick of the next table entry and the summary accumulators of an instance are one McSlot in an LDS
// block of their own (never lds_mid, which the core and the fallback use), one slot per lane group of the wavefront.  Every lane of a
// group reads and rewrites the cursor words with the same values (the state it pushes is group-uniform), lane 0 alone folds the
// summary: no lane reads what another one wrote.
//   push: s.xd, s.yd, s.zd += dv, one add per component and entry, in table order, BEFORE the bookkeeping of the tick (which does not
//     read the velocity) -- so the pre-tick state a deferred instance parks already holds that tick's push;
//   resume (FB = true): the cursor starts past every entry with tick <= the park tick (they were consumed by the first launch), the
//     partial summary the first launch left in summary[gi] is reloaded, and the record of a fallback tick -- written by tick_affine_body
//     through memory -- goes to the handle's scratch record mc.fbrec[gi], whether or not the tick is recorded; from there it is copied
//     to the row the stride gives it and folded into the summary.
struct RolloutMc {
    const ismpc_push* pushes; int n_push;      // batch x n_push, instance-major (NULL with n_push = 0)
    int stride;                                // tick t goes to row (t + 1) / stride - 1 when (t + 1) % stride == 0
    ismpc_rollout_summary* summary;            // NULL, or batch records
    ismpc_tick_out* fbrec;                     // batch scratch records (handle-owned): where the resume launch's fallback ticks leave their record
};
struct McSlot { double zmin, zmax, vx, vy; int status_or, first_err, err_ticks, fb_ticks, cursor, next_tick; };      // 56 bytes
typedef volatile __attribute__((address_space(3))) McSlot LdsSlot;      // ... addressed as LDS (ds_read / ds_write, never a flat access) and volatile: the
// optimiser would otherwise promote the slot to registers for the length of the tick loop, which is what it exists to avoid.  S below: McSlot or LdsSlot
template <class S> __device__ __forceinline__ void mc_summary_init(S* a)
{
    a->zmin = INFINITY; a->zmax = -INFINITY; a->vx = 0.0; a->vy = 0.0;
    a->status_or = 0; a->first_err = -1; a->err_ticks = 0; a->fb_ticks = 0;
}
template <class S> __device__ __forceinline__ void mc_summary_load(S* a, const ismpc_rollout_summary* s)
{
    a->zmin = s->com_z_min; a->zmax = s->com_z_max; a->vx = s->max_abs_vel[0]; a->vy = s->max_abs_vel[1];
    a->status_or = s->status_or; a->first_err = s->first_error_tick; a->err_ticks = s->error_ticks; a->fb_ticks = s->fallback_ticks;
}
template <class S> __device__ __forceinline__ void mc_summary_store(ismpc_rollout_summary* s, const S* a)
{
    s->status_or = a->status_or; s->first_error_tick = a->first_err; s->error_ticks = a->err_ticks; s->fallback_ticks = a->fb_ticks;
    s->com_z_min = a->zmin; s->com_z_max = a->zmax; s->max_abs_vel[0] = a->vx; s->max_abs_vel[1] = a->vy;
}
// one tick's record into the summary (fmin / fmax: independent of the order, NaN records leave the extrema alone)
template <class S> __device__ __forceinline__ void mc_summary_fold(S* a, int status, double z, double xd, double yd, int t)
{
    a->status_or |= status;
    if (status & ISMPC_ST_ERROR_MASK) { if (a->first_err < 0) a->first_err = t; a->err_ticks += 1; }
    if (status & ISMPC_ST_Z_INEQ_ACTIVE) a->fb_ticks += 1;
    a->zmin = fmin(a->zmin, z); a->zmax = fmax(a->zmax, z);
    a->vx = fmax(a->vx, fabs(xd)); a->vy = fmax(a->vy, fabs(yd));
}
// the slot of lane group `grp` of wavefront `wv` (MC = false: no LDS, no slot)
template <bool MC, int IPW> __device__ __forceinline__ LdsSlot* mc_slot_of(int wv, int grp)
{
    if constexpr (MC) { __shared__ McSlot mc_lds[ISMPC_QUAD_WAVES * IPW]; return (LdsSlot*)(mc_lds + wv * IPW + grp); }
    else return nullptr;
}
// the first entry at or after `cur` of an instance's table that the cursor rule has not passed once tick `past` is done
__device__ __forceinline__ int mc_cursor_after(const ismpc_push* pt, int np, int cur, int past)
{
    while (cur < np && pt[cur].tick <= past) ++cur;
    return cur;
}
template <int R, int LPI, int RW, bool FB, int SW = 0, bool MC = false>
__global__ __launch_bounds__(64 * ISMPC_QUAD_WAVES, 2)
void ismpc_rollout_quad(const DevConst c, ismpc_tick_in* state, ismpc_tick_out* __restrict__ traj, int batch, int first_frame, int ticks,
                        int* __restrict__ stop_tick, int launch_id, const RolloutMc mc)
{
    constexpr int IPW = 64 / LPI;
    __shared__ double2 lds_mid[ISMPC_QUAD_WAVES][FB ? wave_lds_double2_fb<R, LPI>() : wave_lds_double2<R, LPI>()];
    const int lane = threadIdx.x & 63, li = lane & (LPI - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = blockIdx.x * ISMPC_QUAD_WAVES + wv;
    LdsSlot* const slot = mc_slot_of<MC, IPW>(wv, lane / LPI);
    if constexpr (FB) { if (*(volatile int*)(c.zflag + 2) == 0) return; }      // nothing parked (workgroup-uniform: the first launch is done)
    const int nwork = FB ? batch : (batch + IPW - 1) / IPW;          // FB: one instance per wavefront (every group computes it, group 0 stores)
    for (int work = wave; work < nwork; work += FB ? (int)gridDim.x * ISMPC_QUAD_WAVES : nwork) {
        const int gi_raw = FB ? work : work * IPW + lane / LPI;
        const bool valid = FB ? (lane < LPI) : (gi_raw < batch);
        const int gi = (gi_raw < batch) ? gi_raw : batch - 1;
        int t0 = 0;
        if constexpr (FB) { t0 = stop_tick[gi]; if (t0 < 0) continue; }
        ismpc_tick_in* rec = state + gi;
        QState s;
        load_state(rec, s);
        s.ps = SW ? record_index<SW>(c, rec->reserved) : 0;            // sweep handles: the instance's parameter set; multi-plan handles: its (set, plan) pair
        const double* ftsp_t = SW == 2 ? c.sets[max(s.ps, 0)].ftsp_t : c.ftsp_t;
        bool alive = true;                                              // FB = false: false once the instance is parked
        int stopped = -1;
        int phase = 0, row = 0;                                         // MC: ticks since the last recorded one, next trajectory row (wave-uniform)
        if constexpr (MC) {
            // a padding group (FB = false, gi clamped) has no table: it is never pushed and, like everything of it, never stored
            const int np = (FB || valid) ? mc.n_push : 0;
            const ismpc_push* pt = mc.pushes + (size_t)gi * mc.n_push;
            const int cur = FB ? mc_cursor_after(pt, np, 0, t0) : 0;      // (the resume launch: past what the first launch consumed)
            slot->cursor = cur; slot->next_tick = cur < np ? pt[cur].tick : INT32_MAX;
            if (FB && mc.summary) mc_summary_load(slot, mc.summary + gi); else mc_summary_init(slot);
            if constexpr (FB) { const int t0u = __builtin_amdgcn_readfirstlane(t0); phase = t0u % mc.stride; row = t0u / mc.stride; }
        }
        for (int t = t0; t < ticks; ++t) {
            const int frame = first_frame + t;
            bool rec_t = true; int trow = t;                            // is this tick recorded, and in which row (MC = false: every tick, row t)
            if constexpr (MC) {
                if (slot->next_tick <= t) {                             // the cursor rule of ismpc_rollout_mc_device (include/ismpc.h)
                    const ismpc_push* pt = mc.pushes + (size_t)gi * mc.n_push;
                    int cur = slot->cursor, nt;
                    do {
                        if (pt[cur].tick == t) { s.xd += pt[cur].dv[0]; s.yd += pt[cur].dv[1]; s.zd += pt[cur].dv[2]; }
                        ++cur;
                        nt = cur < mc.n_push ? pt[cur].tick : INT32_MAX;
                    } while (nt <= t);
                    slot->cursor = cur; slot->next_tick = nt;
                }
                ++phase; rec_t = phase == mc.stride;
                if (rec_t) { phase = 0; trow = row; ++row; }
            }
            // caller bookkeeping in front of solve(): Controller.cpp:297-304 (enabled) and :310
            const Walk before = s.w;
            advance_walk(c, ftsp_t, s.w, frame);
            QOut o;
            const bool def = tick_group_core<R, LPI, SW, false>(c, lane, s, o, nullptr, lds_mid[wv], true);      // (no mask here: see tick_group_core)
            const bool park = def && alive;
            if constexpr (MC) {
                if (li == 0 && valid && alive && !def) {
                    if (rec_t && traj) store_record(traj + (size_t)trow * batch + gi, o);
                    if (mc.summary) mc_summary_fold(slot, o.status, o.z, o.xd, o.yd, t);
                }
            } else
            if (li == 0 && valid && alive && !def && traj) store_record(traj + (size_t)t * batch + gi, o);
            // a deferred instance: its pre-tick state goes to memory (FB = false: to stay there; FB = true: for the fallback body)
            if (park && valid && li == 0) store_state(rec, s, before);
            if constexpr (!FB) {
                if (park) { alive = false; stopped = t; }
            }
            // feedback (Controller.cpp:346-348) and counters (:503-504), in registers; lane 0 of the group holds the result
            s.x = Grp<LPI>::bcast0(o.x); s.y = Grp<LPI>::bcast0(o.y); s.z = Grp<LPI>::bcast0(o.z);
            s.xd = Grp<LPI>::bcast0(o.xd); s.yd = Grp<LPI>::bcast0(o.yd); s.zd = Grp<LPI>::bcast0(o.zd);
            s.w.ctl = s.w.ctl + 1;
            s.w.mpc = (int)floor(s.w.ctl * c.cdt / c.dt);
            if constexpr (FB) {
                if (__builtin_amdgcn_ballot_w64(def && valid) != 0ull) {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    // the row the fallback body writes its record to (MC: always the scratch record mc.fbrec[gi]; copied and folded below)
                    ismpc_tick_out* frow = traj ? traj + (size_t)t * batch : nullptr;
                    if constexpr (MC) frow = mc.fbrec;
                    // the fallback's working window.  MC: the pointer goes through an empty asm, i.e. the body sees a flat pointer it knows nothing about --
                    // with a second LDS block in the kernel the ROCm 7.2 gfx950 backend otherwise folds the body's null test of the window into an
                    // instruction its own verifier rejects (<13, 8, 2, true, 0, true>: "Illegal instruction detected", V_CMP_NE_U32 0, src_shared_base)
                    double* zwin = reinterpret_cast<double*>(lds_mid[wv]);
                    if constexpr (MC) asm volatile("" : "+v"(zwin));
                    // (FB: one instance per wavefront, its set is wave-uniform and valid -- an invalid one never defers)
                    tick_affine_body<RW, true>(SW ? c.sets[__builtin_amdgcn_readfirstlane(max(s.ps, 0))] : c, gi, lane, nullptr, state,
                                               frow, nullptr, frame, nullptr, 0, nullptr, 0, zwin);
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    load_state(static_cast<const volatile ismpc_tick_in*>(rec), s);
                    if constexpr (MC) {
                        // lane k copies the word it wrote itself (store_record_lanes) to the row the stride gives the tick; lane 0 folds the record
                        const volatile ismpc_tick_out* fr = mc.fbrec + gi;
                        if (rec_t && traj && lane < 10)
                            reinterpret_cast<double*>(traj + (size_t)trow * batch + gi)[lane] = reinterpret_cast<const volatile double*>(fr)[lane];
                        if (mc.summary && li == 0 && valid) mc_summary_fold(slot, fr->status, fr->com_pos[2], fr->com_vel[0], fr->com_vel[1], t);
                    }
                }
            }
        }
        if (li == 0 && valid) {
            if (alive) store_state(rec, s, s.w);
            if constexpr (MC) { if (mc.summary) mc_summary_store(mc.summary + gi, slot); }      // (FB = false, parked: the ticks before the park)
            if constexpr (!FB) {
                stop_tick[gi] = stopped;
                if (stopped >= 0) atomicAdd(c.zflag + 2, 1);
            }
        }
    }
    if constexpr (FB) {      // the last resume workgroup zeroes the parked count for the next rollout (see DevConst::zflag)
        __syncthreads();
        if (threadIdx.x == 0 && atomicAdd(c.zflag + 3, 1) == (int)gridDim.x - 1) { c.zflag[2] = 0; c.zflag[3] = 0; __threadfence(); }
    }
}

// The same semantics for handles that run their closed loop as one launch per tick (ISMPC_ROLLOUT=host, N > 128, the dense path): two
// elementwise kernels around the tick's launch, one thread per instance.  ismpc_mc_push applies tick t's entries to the state records --
// the cursor is rebuilt from the table (where it stands once tick t - 1 is done), so nothing is carried between launches;
// ismpc_mc_fold folds the tick's records into the summaries (recs == NULL: sets them to the empty summary).
__global__ __launch_bounds__(256) void ismpc_mc_push(ismpc_tick_in* state, int batch, const ismpc_push* __restrict__ pushes, int n_push, int t)
{
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= batch) return;
    const ismpc_push* pt = pushes + (size_t)gi * n_push;
    double* v = state[gi].com_vel;
    for (int cur = mc_cursor_after(pt, n_push, 0, t - 1); cur < n_push && pt[cur].tick <= t; ++cur)
        if (pt[cur].tick == t) { v[0] += pt[cur].dv[0]; v[1] += pt[cur].dv[1]; v[2] += pt[cur].dv[2]; }
}
__global__ __launch_bounds__(256) void ismpc_mc_fold(const ismpc_tick_out* __restrict__ recs, int batch, ismpc_rollout_summary* summary, int t)
{
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= batch) return;
    McSlot a;
    if (recs) {
        mc_summary_load(&a, summary + gi);
        mc_summary_fold(&a, recs[gi].status, recs[gi].com_pos[2], recs[gi].com_vel[0], recs[gi].com_vel[1], t);
    } else mc_summary_init(&a);
    mc_summary_store(summary + gi, &a);
}

// ---- ismpc_sweep_bind: counting sort of the instances of a batch by the record they name -- their parameter set (SW = 1) or, for a multi-plan
// handle (SW = 2), their (set, plan) pair, set-major: the lane groups of a wavefront then read one set's tables AND one plan's window.  The
// last bucket takes the instances that name no record.
template <int SW> __device__ __forceinline__ int sort_bucket(const DevConst& c, int reserved)
{
    const int k = record_index<SW>(c, reserved);
    return k >= 0 ? k : c.nsets * (SW == 2 ? c.nplans : 1);
}
template <int SW>
__global__ __launch_bounds__(256) void sweep_sort_hist(const DevConst c, const ismpc_tick_in* __restrict__ in, int batch, int* __restrict__ counts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    atomicAdd(counts + sort_bucket<SW>(c, in[i].reserved), 1);
}
// exclusive scan of counts[0 .. n) in place (one workgroup; n <= 65 536 + 1 sets, or 2^24 + 1 (set, plan) pairs of a multi-plan handle): counts[k] becomes the first slot of bucket k
__global__ __launch_bounds__(256) void sweep_sort_scan(int* __restrict__ counts, int n)
{
    __shared__ int part[256];
    const int tid = threadIdx.x, per = (n + 255) / 256, lo = tid * per, hi = min(lo + per, n);
    int s = 0;
    for (int k = lo; k < hi; ++k) s += counts[k];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int k = 0; k < 256; ++k) { const int v = part[k]; part[k] = run; run += v; } }
    __syncthreads();
    int run = part[tid];
    for (int k = lo; k < hi; ++k) { const int v = counts[k]; counts[k] = run; run += v; }
}
template <int SW>
__global__ __launch_bounds__(256) void sweep_sort_scatter(const DevConst c, const ismpc_tick_in* __restrict__ in, int batch, int* __restrict__ cursor, int* __restrict__ order)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    order[atomicAdd(cursor + sort_bucket<SW>(c, in[i].reserved), 1)] = i;      // (the order INSIDE a bucket is whatever the atomics give: no result depends on it)
}

}  // namespace
