// Formulation B, part 1 of 4 of the translation unit ismpc_hip.hip (which sets the floating-point contraction for all parts):
// what every kernel family shares -- the launch constants (DevConst), the caller bookkeeping in front of a tick (Walk,
// load_walk, gate_tick), small device functions, the per-instance registers of the lane-group kernels (QState / QOut) with
// their record stores, and the -DISMPC_STAMPS instrumentation.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ismpc_tables.hpp"
#include "ismpc_wave_prims.hpp"

namespace {

using namespace ismpc_wave;

struct DevConst {
    int N, NP, NPs, S, F, nmid, npat, Fmax, rows, tick_divisor;
    double dt, cdt, mass, g, h_des, half_run, half_first, q_p, q_u, q_v, z_lo, z_hi, gate, eta;
    double inv_mass, dt_over_mass, inv_eta, sim_div, cdt_over_dt;   // 1/m, dt/m (B_z), 1/eta (C_sc), dt/cdt, cdt/dt: uniform divisions hoisted to the host
    const double *Hinv, *W, *midx, *midy, *midz, *tailx, *taily, *ftsp_t;
    const int *e_lo, *ne;
    // affine form of the vertical stage (ismpc_tables.hpp)
    const double *vtab, *tz, *tg, *dU, *SdU, *Wt, *SW;
    int flat;
    // inequality fallback (0 <= S u <= 1e4 active)
    const double *HSt, *SHSt;
    const DevConst* sets; int nsets;  // parameter sweeps (ismpc_create_sweep): one record per parameter set, its own tables and scalars; the
                                      // instance's record names its set (ismpc_tick_in.reserved).  NULL / 0 for a plain handle
    int nplans;                       // multi-plan handles (ismpc_create_plans): `sets` holds one record per (set, plan) PAIR, set-major -- the set's
                                      // record with the plan's midpoint tables, step timings and the pair's tails -- and reserved is
                                      // ISMPC_RESERVED(set, plan).  0 otherwise
    const int* order;                 // sweeps, after ismpc_sweep_bind: the instances of the bound batch sorted by parameter set.  Slot g of the
                                      // launch runs instance order[g], so the lane groups of a wavefront read ONE set's tables, and workgroup b
                                      // takes the slots of virtual block sweep_vblock(b): the workgroups an XCD receives (b mod 8) cover one
                                      // contiguous eighth of the sorted batch -- K / 8 sets' tables per L2 instead of all K.  NULL: slot g = instance g
    int* zflag;                       // four self-resetting counters (zeroed once, at ismpc_create): [0] entries in the deferred list of the
                                      // running two-launch step, [1] fallback workgroups done with it, [2] instances an in-kernel rollout
                                      // parked for its resume launch, [3] resume workgroups done.  The consumer launch exits at once on a
                                      // zero count; otherwise its LAST workgroup zeroes the pair again -- so the counters are valid whatever
                                      // launched before (a rollout between two ticks, hipGraph replays of one captured step: the count does
                                      // not depend on launch ids and no memset sits outside a captured step)
    int* zseen;                       // id of the last launch that deferred an instance, in a word of host memory (written, never read, by the device): how the host picks the launch form
    double* zpool; int* zbusy;        // active-set fallback: slots of zstride doubles (G^-1 cap x cap + per-entry vectors), one lock word per slot
    int zslots, zcap, zldsq; size_t zstride;   // zldsq: entries the fallback keeps in its LDS window before it moves to a slot (Z_LDS_Q; ISMPC_Z_LDS_Q lowers it: tests)
    // sample-major copies for ismpc_tick_quad: a lane's R samples are one contiguous run (16-byte loads, one base address)
    const double *vq;                 // (npat+1) x NT x 6 : U0,Ua,Ub,SU0,SUa,SUb per sample
    const double *tzg;                // NT x 2 : tz, tg per sample
    const double *midxy;              // nmid x 2 : midx, midy per sample
    // the same tables laid out for the lane-group kernels' shape (R samples per lane, LPI lanes per instance), so that one
    // wave-wide load instruction reads LPI x 16 contiguous bytes per instance (a lane's samples are NOT contiguous here):
    const double *vqT;                // (npat+1) x R x 3 x LPI double2 : pair k of sample li*R + r at [((p R + r) 3 + k) LPI + li]
    const double *tzgT;               // R x LPI double2 : (tz, tg) of sample li*R + r at [r LPI + li]
};

struct M2 { double a, b, c, d; };   // [a b; c d]
__device__ __forceinline__ M2 mul(const M2& x, const M2& y)
{
    M2 r;
    r.a = fma(x.a, y.a, x.b * y.c); r.b = fma(x.a, y.b, x.b * y.d);
    r.c = fma(x.c, y.a, x.d * y.c); r.d = fma(x.c, y.b, x.d * y.d);
    return r;
}
template <int LANE>
__device__ __forceinline__ M2 readlane_m2(const M2& y)
{
    return (M2){readlane64<LANE>(y.a), readlane64<LANE>(y.b), readlane64<LANE>(y.c), readlane64<LANE>(y.d)};
}

// P = sinh(x)/x and Q = (cosh(x)-1)/x^2 as Taylor series in w = x^2, in two Horner halves.  Degree 7 (taylor_high, then taylor_low) is
// exact to < 1 ulp for w <= 0.25 (next term 4e-20); degree 3 (taylor_low from TAYLOR_P3, TAYLOR_Q3) for w <= 0.004 (next term w^4/9! <=
// 7e-16 relative to 1) -- and w = lambda dt^2 is <= 0.0025 on a physical gait (lambda <= 25 at dt = 0.01).
constexpr double TAYLOR_P3 = 1.0 / 5040.0, TAYLOR_Q3 = 1.0 / 40320.0;     // 1/7!, 1/8!: where degree 3 starts
__device__ __forceinline__ void taylor_high(double w, double& P, double& Q)
{
    P = 1.0 / 1307674368000.0;                  Q = 1.0 / 20922789888000.0;             // 1/15!, 1/16!
    P = fma(P, w, 1.0 / 6227020800.0);          Q = fma(Q, w, 1.0 / 87178291200.0);     // 1/13!, 1/14!
    P = fma(P, w, 1.0 / 39916800.0);            Q = fma(Q, w, 1.0 / 479001600.0);       // 1/11!, 1/12!
    P = fma(P, w, 1.0 / 362880.0);              Q = fma(Q, w, 1.0 / 3628800.0);         // 1/9!, 1/10!
    P = fma(P, w, TAYLOR_P3);                   Q = fma(Q, w, TAYLOR_Q3);
}
__device__ __forceinline__ void taylor_low(double w, double& P, double& Q)
{
    P = fma(P, w, 1.0 / 120.0);                 Q = fma(Q, w, 1.0 / 720.0);             // 1/5!, 1/6!
    P = fma(P, w, 1.0 / 6.0);                   Q = fma(Q, w, 1.0 / 24.0);              // 1/3!, 1/4!
    P = fma(P, w, 1.0);                         Q = fma(Q, w, 0.5);
}
// ... beyond w = 0.25 (lambda dt^2 > 1/4: never on a physical gait) libm
__device__ __forceinline__ void sinhc_coshc(double w, double& P, double& Q)
{
    if (__builtin_expect(w <= 0.25, 1)) { taylor_high(w, P, Q); taylor_low(w, P, Q); }
    else {
        const double x = sqrt(w);
        P = sinh(x) / x;
        Q = (cosh(x) - 1.0) / w;
    }
}
// The entries of A_j, B_j (MPCSolver.cpp:353-361) that differ from 0 / 1: ch1 = cosh(x) - 1 = w Q, s1 = sinh(x) / sqrt(lambda) = dt P,
// s2 = sqrt(lambda) sinh(x) = lambda dt P -- from the series, and from libm for w > 0.25
__device__ __forceinline__ void ab_series(double w, double dtn, double le, double P, double Q, double& ch1, double& s1, double& s2)
{
    ch1 = w * Q; s1 = dtn * P; s2 = le * s1;
}
__device__ __forceinline__ void ab_libm(double w, double dtn, double le, double& ch1, double& s1, double& s2)
{
    const double x = sqrt(w);
    ch1 = cosh(x) - 1.0; s1 = dtn * (sinh(x) / x); s2 = le * s1;
}

// Per-launch scratch of the inequality fallback of the two-launch form: the LIST of deferred instances (batch ints).  The per-tick
// kernel appends an instance under the handle's counter DevConst::zflag[0]; the fallback launch behind it walks exactly those entries
// (scanning 65 536 marks with 256 wavefronts cost 0.5 ms whenever anything was deferred) and its last workgroup zeroes the counter.
__host__ __device__ inline size_t zscratch_bytes(int batch) { return 4 * (size_t)batch + 16; }
__device__ __forceinline__ int* zlist_of(unsigned char* zmark, int) { return reinterpret_cast<int*>(zmark); }
// Caller bookkeeping in front of solve(): Controller.cpp:297-304 (enabled) and :310.
struct Walk { double sim; int mpc, ctl, fc; };
// ... as the in-kernel closed loop applies it before tick `frame` (ftsp_t: the step timings of the instance's plan -- c.ftsp_t unless
// the lanes of a wavefront walk different plans).  load_walk below states the same rule itself: calling this from it costs
// ismpc_tick_dense<2, 16> a VGPR.
__device__ __forceinline__ void advance_walk(const DevConst& c, const double* ftsp_t, Walk& w, int frame)
{
    if (w.fc >= 0 && w.fc < c.rows && w.sim >= ftsp_t[w.fc] - 1) { w.ctl = 0; w.mpc = 0; w.fc = w.fc + 1; }
    w.sim = (double)frame;
}
template <class Rec> __device__ __forceinline__ Walk read_walk(Rec* rec) { return (Walk){rec->simulation_time, rec->mpc_iter, rec->control_iter, rec->footstep_counter}; }
// the bookkeeping a tick runs with: the record's, advanced when the tick is one of a host-driven closed loop (rollout_frame >= 0)
__device__ __forceinline__ Walk load_walk(const DevConst& c, const double* ftsp_t, const ismpc_tick_in* rec, int rollout_frame)
{
    Walk w = read_walk(rec);
    if (rollout_frame >= 0) {
        if (w.fc >= 0 && w.fc < c.rows && w.sim >= ftsp_t[w.fc] - 1) { w.ctl = 0; w.mpc = 0; w.fc = w.fc + 1; }
        w.sim = (double)rollout_frame;
    }
    return w;
}
__device__ __forceinline__ Walk load_walk(const DevConst& c, const ismpc_tick_in* rec, int rollout_frame) { return load_walk(c, c.ftsp_t, rec, rollout_frame); }
// SW, the compile-time form of a kernel: 0 = plain handle, 1 = parameter sweep, 2 = multi-plan handle.  The record in c.sets that
// ismpc_tick_in.reserved names: the set (SW = 1) or the (set, plan) pair (SW = 2); -1 when it names none.
template <int SW> __device__ __forceinline__ int record_index(const DevConst& c, int reserved)
{
    if constexpr (SW == 2) {
        const int set = reserved & 0xffff, plan = reserved >> 16;
        return (reserved >= 0 && set < c.nsets && plan < c.nplans) ? set * c.nplans + plan : -1;
    } else return (reserved >= 0 && reserved < c.nsets) ? reserved : -1;
}
// 0 = run the tick, else the pass-through status (MPCSolver.cpp:214; index range of :259,381)
// Both cold cases are uniform over the launch: the remainder sequence sits behind a scalar branch (x % 1 = 0), and with BRANCH_DIV so does the
// division sequence at mpc_dt = control_dt -- the empty asm keeps it there, a plain conditional is if-converted back into divide-and-select.
// BRANCH_DIV is the lane-group kernels' alone: in the affine and dense kernels the split block costs registers (ismpc_tick_affine<2, 2>: 55 -> 74
// VGPRs, eight wavefronts per SIMD -> six), and they are not bound by the instructions they issue.
template <bool BRANCH_DIV = false>
__device__ __forceinline__ int gate_tick(const DevConst& c, const Walk& w, int& idx)
{
    idx = 0;
    if (c.tick_divisor != 1 && (w.ctl % c.tick_divisor) != 0) return ISMPC_ST_TICK_SKIPPED;
    double t = w.sim;
    if constexpr (BRANCH_DIV) { if (c.sim_div != 1.0) { t = w.sim / c.sim_div; asm volatile("" : "+v"(t)); } }
    else t = (c.sim_div == 1.0) ? w.sim : w.sim / c.sim_div;
    if (!(t > -1.0) || !(t < 2.0e9)) return ISMPC_ST_BAD_INDEX;
    idx = (int)t;
    if (idx < 0 || idx + 2 * c.N > c.nmid || w.mpc < 0) return ISMPC_ST_BAD_INDEX;
    return 0;
}

// 1/x to rounding error: v_rcp_f64 + two Newton steps (the IEEE division sequence is about three times as long)
__device__ __forceinline__ double frcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

// Slack of the bounds on S u, beyond rounding (MPCSolver.cpp:158-160)
__device__ __forceinline__ double z_tol(double bound) { return 1e-11 * fmax(1.0, fabs(bound)); }
// the decision variable of a sample: mid + sg sign(a) min(tau |a|, h)
__device__ __forceinline__ double box_move(double sg, double a, double tau, double h, double mid)
{
    const double sa = (a < 0.0) ? -1.0 : 1.0;
    return fma(sg * sa, (fabs(a) > 0.0) ? fmin(tau * fabs(a), h) : 0.0, mid);
}
// Integration of the vertical axis (MPCSolver.cpp:274-278) ...
__device__ __forceinline__ void integrate_z(const DevConst& c, double dt_over_mass, double h_des, double z0, double zd0, double uz0, double& z, double& zd, int& status)
{
    z = fma(c.dt, zd0, z0);
    zd = fma(dt_over_mass, uz0, zd0) - c.dt * c.g;
    if (isnan(z)) { z = h_des; status |= ISMPC_ST_Z_NAN; }
    if (isnan(zd)) { zd = 0.0; status |= ISMPC_ST_Z_NAN; }
}
// ... and of a horizontal one with A(lambda_0) = [A0a, A0b; A0c, A0a], B(lambda_0) = [1 - A0a, -A0c] (MPCSolver.cpp:406-422)
__device__ __forceinline__ void integrate_xy(double A0a, double A0b, double A0c, double x0, double xd0, double u0, double& x, double& xd)
{
    x  = fma(1.0 - A0a, u0, fma(A0a, x0, A0b * xd0));
    xd = fma(-A0c, u0, fma(A0c, x0, A0a * xd0));
}

// -DISMPC_STAMPS (diagnostic build, scripts/stamps_b.py): wall-clock stamps (s_memrealtime, 100 MHz) of every wavefront of the
// per-tick lane-group kernels at a few points of the tick (words 0..5 of its eight) and the hardware slot it ran in (word 6); written to a
// buffer nothing else reads.
#ifdef ISMPC_STAMPS
__device__ unsigned long long g_stamps[16384 * 8];
__device__ __forceinline__ unsigned long long stamp_now()
{
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
// where the wavefront ran (scripts/slot_timeline.py): HW_ID (wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]) in the low word, XCC_ID above it
__device__ __forceinline__ unsigned long long stamp_where()
{
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(hw), "=s"(xcc));
    return (unsigned long long)hw | ((unsigned long long)xcc << 32);
}
#define STAMP_WHERE do { if (g_stamp_wave >= 0 && g_stamp_wave < 16384) { const unsigned long long w_ = stamp_where(); if ((threadIdx.x & 63) == 0) g_stamps[g_stamp_wave * 8 + 6] = w_; } } while (0)
#define STAMP(k_) do { if (g_stamp_wave >= 0 && g_stamp_wave < 16384) { const unsigned long long t_ = stamp_now(); if ((threadIdx.x & 63) == 0) g_stamps[g_stamp_wave * 8 + (k_)] = t_; } } while (0)
#define STAMP_DECL const int g_stamp_wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)
#else
#define STAMP(k_) do {} while (0)
#define STAMP_WHERE do {} while (0)
#define STAMP_DECL do {} while (0)
#endif

// What one instance carries from tick to tick (group-uniform: every lane of the group holds the same values) and what a tick
// produces (valid in lane 0 of the group).
struct QState { double x, y, z, xd, yd, zd; Walk w; int ps; };     // ps: the instance's record in c.sets (sweep handles: its parameter set; multi-plan handles: its (set, plan) pair; -1 = invalid)
struct QOut { double x, y, z, xd, yd, zd, uz0, ux0, uy0; int status, itx, ity; };

// (Rec: const ismpc_tick_in, or a volatile one where another wavefront's code wrote it; ps is the caller's)
template <class Rec> __device__ __forceinline__ void load_com(Rec* rec, QState& s)
{
    s.x = rec->com_pos[0]; s.y = rec->com_pos[1]; s.z = rec->com_pos[2];
    s.xd = rec->com_vel[0]; s.yd = rec->com_vel[1]; s.zd = rec->com_vel[2];
}
template <class Rec> __device__ __forceinline__ void load_state(Rec* rec, QState& s)
{
    s.w = read_walk(rec);
    load_com(rec, s);
}
__device__ __forceinline__ void store_state(ismpc_tick_in* rec, const QState& s, const Walk& w)
{
    rec->com_pos[0] = s.x; rec->com_pos[1] = s.y; rec->com_pos[2] = s.z;
    rec->com_vel[0] = s.xd; rec->com_vel[1] = s.yd; rec->com_vel[2] = s.zd;
    rec->simulation_time = w.sim; rec->mpc_iter = w.mpc; rec->control_iter = w.ctl; rec->footstep_counter = w.fc;
}
__device__ __forceinline__ void store_record(ismpc_tick_out* __restrict__ rec, const QOut& o)
{
    double2* o2 = reinterpret_cast<double2*>(rec);
    const long long packed = (long long)(unsigned)o.status | ((long long)(unsigned)((o.itx & 255) | ((o.ity & 255) << 8)) << 32);
    o2[0] = make_double2(o.x, o.y); o2[1] = make_double2(o.z, o.xd); o2[2] = make_double2(o.yd, o.zd);
    o2[3] = make_double2(o.uz0, o.ux0); o2[4] = make_double2(o.uy0, __longlong_as_double(packed));
}
// The same 80-byte record from a wavefront that holds the result in every lane: lanes 0..9 store one 8-byte word each (zits: iterations
// of the inequality fallback)
__device__ __forceinline__ void store_record_lanes(ismpc_tick_out* __restrict__ out, int gi, int lane, const QOut& o, int zits)
{
    double word = 0.0;
    const long long packed = (long long)(unsigned)o.status | ((long long)(unsigned)((o.itx & 255) | ((o.ity & 255) << 8) | ((zits & 255) << 16)) << 32);
    switch (lane) {
        case 0: word = o.x; break;   case 1: word = o.y; break;   case 2: word = o.z; break;
        case 3: word = o.xd; break;  case 4: word = o.yd; break;  case 5: word = o.zd; break;
        case 6: word = o.uz0; break; case 7: word = o.ux0; break; case 8: word = o.uy0; break;
        case 9: word = __longlong_as_double(packed); break;
        default: break;
    }
    if (out && lane < 10) reinterpret_cast<double*>(out + gi)[lane] = word;
}
// Controller.cpp:346-348 (feed the output back), :503-504 (advance the counters)
__device__ __forceinline__ void store_feedback(const DevConst& c, ismpc_tick_in* __restrict__ st, const QOut& o, const Walk& w)
{
    st->com_pos[0] = o.x; st->com_pos[1] = o.y; st->com_pos[2] = o.z;
    st->com_vel[0] = o.xd; st->com_vel[1] = o.yd; st->com_vel[2] = o.zd;
    st->simulation_time = w.sim;
    const int ctl = w.ctl + 1;
    st->control_iter = ctl;
    st->mpc_iter = (int)floor(ctl * c.cdt / c.dt);     // as written at Controller.cpp:504: 29*0.01/0.01 floors to 28, and parity keeps that
    st->footstep_counter = w.fc;
}

}  // namespace
