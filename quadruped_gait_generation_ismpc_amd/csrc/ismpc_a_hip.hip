// Formulation A (classic ISMPC with footstep adaptation) on gfx950: kernels + the C ABI of include/ismpc_a.h.  The per-axis QP and
// the method (a dual active-set solve in range-space form that never builds a matrix over the variables) are stated at the top of
// ismpc_a_wave.hpp; DESIGN.md section 2.6.  This file is one translation unit over two kernel headers; the wave kernels are units of their own:
//
//   ismpc_a_dev.hpp         DevA (the handle's constants), PiPre, WaveLaunch: what the units of Formulation A share
//   ismpc_a_wave.hpp        ismpc_a_tick_wave<Real, RL, F, PI>, the DEFAULT: one wavefront per QP, 3 <= F <= 6; instantiated per
//                           rows-per-lane value in ismpc_a_wave_rl2.hip, _rl3.hip, _rl4.hip (launch_wave_rl*)
//   ismpc_a_block.hpp       ismpc_a_tick_kernel: one workgroup per QP; every other F, and ISMPC_A_KERNEL=block (A/B)
//   ismpc_a_feet.hpp        ismpc_a_feet_kernel (swing-foot re-placement after a tick), ismpc_a_feet_fill, ismpc_a_feet_fill_inst
//   ismpc_a_feet_files.hpp  ismpc_a_feet_summary_kernel (a batch's foot plans against the base plans), ismpc_a_foot_trajectories_kernel (the
//                           four foot files of every instance, the host writer's bits)
//   ismpc_a_plans.hpp       ismpc_a_plan_table_kernel (the plan generators on the device: every plan of a plan-table handle in one launch,
//                           the host's ismpc_a_plan to the bit)
//   ismpc_a_horizon.hpp     ismpc_a_predict_kernel (the predicted CoM / ZMP horizon of a tick from its whole decision; the decision itself is
//                           stored by the Horizon<> instantiations of the wave kernel, ismpc_a_wave_rl*_hz.hip, and ismpc_a_tick_kernel<true>)
//   ismpc_wave_prims.hpp    wavefront prefix sum (shared with Formulation B)
//   ismpc_host.hpp          device guard, early return on a HIP error, growth of scratch (shared by the three ABIs)
//   this file               the error string; host geometry (linspace_m, centreline, ismpc_a_plan, ismpc_a_foot_trajectories, the text
//                           writer); ismpc_a_handle and its run-time knobs; the launch path (ismpc_a_tick_prologue, ismpc_a_bucket_by_F,
//                           tick_launch, tick_feet, rollout_a); the disturbed closed loop (ismpc_a_mc_prologue, ismpc_a_mc_fold,
//                           ismpc_a_rollout_mc_device, ismpc_a_rollout_mc_feet_device); ismpc_a_foot_trajectories_device; plan-table handles
//                           (ismpc_a_plan_steps, build_plan_table, ismpc_a_create_plans, ismpc_a_feet_init_plans_device); the extern "C"
//                           entry points
//
// Results are the unique minimiser: validated against the oracle's null-space Goldfarb-Idnani and the
// reference's qpOASES (tests/).  No CPU fallback.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <string>
#include <vector>
#include <array>
#include <new>
#include <algorithm>
#include "ismpc_a_dev.hpp"
#include "ismpc_wave_prims.hpp"
#include "ismpc_host.hpp"
#include "ismpc_a_block.hpp"
#include "ismpc_a_feet.hpp"
#include "ismpc_a_feet_files.hpp"
#include "ismpc_a_plans.hpp"
#include "ismpc_a_horizon.hpp"

namespace {

thread_local std::string g_err_a = "";
int fail_a(int code, const std::string& msg) { g_err_a = msg; return code; }
#define HIP_TRY_A(expr) ISMPC_HIP_TRY(fail_a, expr)
#define ON_DEVICE_A(h_) ISMPC_ON_DEVICE(fail_a, h_)
using ismpc_host::grow_sync;                           // (ISMPC_GROW_ASYNC calls it unqualified)
using DeviceGuardA = ismpc_host::DeviceGuard;          // entry points leave the caller's current device as they found it

// MATLAB linspace(d1, d2, n)
void linspace_m(double d1, double d2, int n, std::vector<double>& y)
{
    y.resize(n);
    const int n1 = n - 1;
    for (int k = 0; k <= n1; ++k) y[k] = d1 + (k * (d2 - d1)) / n1;
    if (n > 0) { y[0] = d1; y[n1] = d2; }
}
// quad_walk_no_plots.m:86-99 (initial) / :540-549 (rebuilt)
void centreline(const std::vector<double>& fs, int step, int ds, int NF, bool initial, std::vector<double>& cl)
{
    cl.clear();
    std::vector<double> lin;
    if (initial) {
        for (int k = 0; k < step - ds; ++k) cl.push_back(fs[0] * 1.0);
        linspace_m(fs[0], fs[1], ds, lin);
        cl.insert(cl.end(), lin.begin(), lin.end());
    } else {
        for (int k = 0; k < step; ++k) cl.push_back(fs[0] * 1.0);
    }
    for (int i = 2; i <= NF - 1; ++i) {
        for (int k = 0; k < step - ds; ++k) cl.push_back(fs[i - 1] * 1.0);
        linspace_m(fs[i - 1], fs[i], ds, lin);
        cl.insert(cl.end(), lin.begin(), lin.end());
    }
}

}  // namespace

struct ismpc_a_handle {
    ismpc_a_params p{};
    DevA c{};
    int device = 0, slots = 0;
    ismpc_a_state* prev = nullptr; int prev_cap = 0;     // copy of the state the tick reads
    FeetParams feet{}; double* feet_base = nullptr;     // swing-foot QPs (ismpc_a_feet_init_device)
    int feet_base_plans = 0;                             // base plans feet_base holds (feet_upload): what ismpc_a_feet_summary_kernel may index
    FeetParamsSet feet_set{}; int feet_plans = 0;        // ... and per base plan (ismpc_a_feet_init_inst_device)
    FeetParams* feet_rules = nullptr;                    // device copy of both: [0, 4) feet_set.p, [4] feet (what the feet kernels read: FeetTab)
    double* plan_tab = nullptr;                          // ismpc_a_create: the centres of up to four base plans (c.tab_x, c.tab_y point into it)
    // plan-table handles (ismpc_a_create_plans): the table the generator kernel wrote (c.tab_x / c.tab_y are its centres) and the records
    bool table = false; double* tab_feet = nullptr; FeetParams* tab_rules = nullptr; float build_ms = 0.0f;
    bool feet_from_table = false;                        // plain feet launches read plan 0 of the table (ismpc_a_feet_init_plans_device), not feet_base
    std::vector<ismpc_a_gait> gaits;
    // what the feet kernels read: per-instance launches any plan of the handle, plain launches plan 0 (the rules of ismpc_a_feet_init_device)
    FeetTab feet_tab(bool per_inst) const
    {
        if (table && (per_inst || feet_from_table)) return FeetTab{tab_rules, tab_feet, per_inst ? c.nplans : 1, plan_table_rows(p.n_gait)};
        return per_inst ? FeetTab{feet_rules, feet_base, feet_plans, feet.rows} : FeetTab{feet_rules + 4, feet_base, 1, feet.rows};
    }
    bool use_wave = true; int wave_blocks = 0;           // structured wavefront-per-QP kernel (default) vs workgroup-per-QP
    int cus = 0, wave_occ[32] = {0};                     // resident workgroups per CU of the wave kernels ([decision stored][F - 3][precision x per-instance])
    ismpc_a::PiPre* pre = nullptr; int pre_cap = 0;       // per-instance launches: the prologue's record per instance
    int* order = nullptr; int order_cap = 0;             // per-instance launches: instance lists by footstep count (4 x cap) + 4 counters
    bool bucket_by_F = false;                            // ISMPC_A_BUCKET=1: one launch per footstep count instead of one launch of the widest kernel
                                                         // (measured slower: 6.2 vs 4.0 ms at 16 384 instances -- four tails of 100-iteration QPs instead of one)
    int precision = 0;                                   // 0: the QPs are solved in fp64, 1: in fp32 (ismpc_a_set_precision)
    DevA* c_dev = nullptr; bool c_dirty = true;          // the constants in device memory (what the wave kernels read), re-sent after a change
    int* work_counter = nullptr;                          // [0] the launch's counter, [1] the fp64 re-solve's, [2] deferred QPs of the fp32 launch
    int resolve_grid = 64;                                // workgroups of the fp64 re-solve launch behind an fp32 launch (ISMPC_A_RESOLVE_GRID)
    int* defer_list = nullptr; int defer_cap = 0; bool defer_off = false;   // fp32 solve: QPs handed to the fp64 instantiation (ISMPC_A_F32_RESOLVE=0: none)
    unsigned long long* hist = nullptr; int hist_cap = 0;   // per-QP working set of the previous tick (closed-loop first guess)
    int claim_chunk = 0;                                  // 0: by shape (tick_launch), else ISMPC_A_CLAIM
    int static_q = 8;                                     // sixteenths of a launch dealt out without atomics (ISMPC_A_STATIC; scripts/claim_sweep.sh:
                                                          // half is +2-12 % on every bench leg, three quarters starts to cost balance)
    bool hist_ticks = false, hist_valid = false;           // use it in plain tick calls too / it holds the previous tick of this batch
    int hist_batch = 0; bool hist_off = false;            // ISMPC_A_HISTORY=0: never (A/B)
    ismpc_a_out* mc = nullptr; int mc_cap = 0;            // disturbed rollouts: per instance an output record for ticks only the summary wants,
                                                          // then (behind mc_cap records) the tick's push, 2 doubles per instance
    hipStream_t last_stream = nullptr; bool used = false; // stream of the previous launch: scratch that outlives a call is re-allocated only
                                                          // after that stream has drained (ismpc_host::grow_sync, inside ISMPC_GROW_ASYNC)
    std::vector<void*> allocs;                            // allocated once, at ismpc_a_create / ismpc_a_add_plan
    std::vector<double> fsx, fsy;
    // the scratch that is re-allocated as batches grow (ismpc_a_reserve, tick_launch, feet_upload): what ismpc_a_destroy frees besides `allocs`
    std::array<void*, 7> scratch() const { return {prev, hist, defer_list, order, pre, feet_base, mc}; }
};

namespace {
template <typename Tp>
int upload_a(ismpc_a_handle* h, const std::vector<Tp>& v, const Tp** dst)
{
    void* p = nullptr;
    HIP_TRY_A(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(Tp)));
    h->allocs.push_back(p);
    if (!v.empty()) HIP_TRY_A(hipMemcpy(p, v.data(), v.size() * sizeof(Tp), hipMemcpyHostToDevice));
    *dst = static_cast<const Tp*>(p);
    return 0;
}

// Run-time knobs, read once at ismpc_a_create; an unset variable leaves the default.  An integer clamped to [lo, hi]:
int clampi(int v, int lo, int hi) { return std::max(lo, std::min(v, hi)); }
void env_int(const char* name, int lo, int hi, int* dst) { if (const char* e = std::getenv(name)) *dst = clampi(std::atoi(e), lo, hi); }
// ... a switch: *dst becomes `nonzero_means` when the value is a non-zero integer and its opposite otherwise
void env_switch(const char* name, bool nonzero_means, bool* dst) { if (const char* e = std::getenv(name)) *dst = (std::atoi(e) != 0) == nonzero_means; }
// ... a word
bool env_is(const char* name, const char* word) { const char* e = std::getenv(name); return e && !std::strcmp(e, word); }

// Per-instance gait parameters: the instances of a batch differ in their footstep count F_i (3..6), and a QP costs what the
// kernel instantiated for its F costs (border of 2F+1 columns, F(F+1)/2 + 2F + 2 Gram sums per block solve).  The instances
// are therefore listed by F_i (order of arrival inside a list is irrelevant: QPs are independent) and each list runs through
// the kernel of its own shape; records the kernel would reject (F out of range ...) go with F = 3 and are flagged there.
__global__ void ismpc_a_bucket_by_F(const ismpc_a_inst* __restrict__ inst, int batch, int Fmax, int* __restrict__ order, int cap, int* __restrict__ counts)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    int f = inst[i].F;
    if (f < 3) f = 3;
    if (f > Fmax) f = 3;
    const int b = f - 3;
    order[(size_t)b * cap + atomicAdd(&counts[b], 1)] = i;
}

// Everything a tick needs before its solver launch, in one launch instead of a copy, a clear and a memset: the snapshot of the
// state the two QPs of an instance read (the solver updates `state` in place), cleared flags of the output records, zeroed
// work counters.  96-byte state records move as six 16-byte words per thread.
// With per-instance gait parameters also the PiPre record of every instance (ismpc_a_dev.hpp).
__global__ void ismpc_a_tick_prologue(const ismpc_a_state* __restrict__ state, ismpc_a_state* __restrict__ prev, ismpc_a_out* out, int batch, int* counters,
                                      const ismpc_a_inst* __restrict__ inst, ismpc_a::PiPre* __restrict__ pre, double grav, double dt, int C, int P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 && counters) counters[i] = 0;
    // the snapshot as one flat, coalesced copy of 16-byte words (a thread per record moved six words 96 bytes apart per wavefront access)
    static_assert(sizeof(ismpc_a_state) % 16 == 0, "state record: whole 16-byte words");
    {
        constexpr int WPR = (int)(sizeof(ismpc_a_state) / 16);
        const double2* src = reinterpret_cast<const double2*>(state);
        double2* dst = reinterpret_cast<double2*>(prev);
        const long long nw = (long long)batch * WPR;
        for (long long w = i; w < nw; w += (long long)gridDim.x * blockDim.x) dst[w] = src[w];
    }
    if (i >= batch) return;
    if (inst && pre) {
        const double height = inst[i].height;
        const double eta = (height > 0) ? sqrt(grav / height) : 1.0;      // (a record the solver rejects: any finite values)
        const double lam = exp(-eta * dt);
        auto ipw = [](double b, int n) { double r = 1.0; while (n > 0) { if (n & 1) r *= b; b *= b; n >>= 1; } return r; };
        const double lamC = ipw(lam, C), lamP = ipw(lam, P);
        const double r1 = 1.0 / (1.0 - lam);
        const double k1c = (1 / eta) * (1 - lam) / (1 - lamC), k2c = dt * 1.0 * lamC;
        ismpc_a::PiPre q;
        q.eta = eta; q.lam = lam; q.lamC = lamC; q.lamP = lamP; q.k1c = k1c; q.k2c = k2c;
        q.A1 = k1c * r1; q.A2 = k1c * k1c / ((1.0 - lam) * (1.0 + lam)); q.B2 = 2.0 * k1c * k2c * r1;
        q.aa = (q.A2 * ((1.0 - lamC) * (1.0 + lamC)) - q.B2 * (1.0 - lamC)) + (double)C * (k2c * k2c);     // = the kernel's sum_{k<C} a_k^2
        const double Qf = (inst[i].Qf > 0) ? inst[i].Qf : 1.0;
        const int step = inst[i].step >= 2 ? inst[i].step : 2, ds = inst[i].ds >= 2 ? inst[i].ds : 2;
        q.sqQf = sqrt(Qf); q.isqQf = 1.0 / sqrt(Qf); q.iQf = 1.0 / Qf; q.ieta = 1.0 / eta;
        q.inv_ds = 1.0 / (double)ds; q.inv_dsm1 = 1.0 / (double)(ds - 1); q.rstep = 1.0f / (float)step; q.pad_ = 0;
        const double ie = 1.0 / lam;
        q.ch = 0.5 * (ie + lam); q.sh = 0.5 * (ie - lam); q.sh_eta = q.sh / eta;
        pre[i] = q;
    }
    if (out) { out[i].status = 0; out[i].active = 0; out[i].iters_x = 0; out[i].iters_y = 0; }
}

// ---- the disturbed closed loop (ismpc_a_rollout_mc_device)
// What tick t of that loop needs beyond a plain tick's prologue.  Nothing is carried from launch to launch but the summary itself.
struct McTick {
    const ismpc_a_push* pushes; int n_push, t;            // the push table (batch x n_push, instance-major) and the tick; NULL: no pushes
    double* push;                                         // batch x 2, the handle's: what the solver launch of tick t reads as `push`
    const ismpc_a_out* last; ismpc_a_rollout_summary* summary;   // output records of tick t - 1 (NULL at t = 0), folded into summary (NULL: none)
};
constexpr size_t MC_BYTES_PER_INSTANCE = sizeof(ismpc_a_out) + 2 * sizeof(double);   // ismpc_a_handle::mc: a record and a push per instance
static_assert(sizeof(ismpc_a_out) % 16 == 0, "the pushes behind the records are stored as 16-byte words");

// The summary of no ticks, and one output record (of tick t) folded into a summary.  fmax: NaN-ignoring and independent of the order,
// so the extrema are np.fmax over the stride-1 trajectory to the bit.
__device__ __forceinline__ ismpc_a_rollout_summary mc_empty_summary()
{
    ismpc_a_rollout_summary s;
    s.status_or = 0; s.first_error_tick = -1; s.error_ticks = 0; s.iter_limit_ticks = 0;
    s.iters_sum_x = 0; s.iters_sum_y = 0; s.max_active_x = 0; s.max_active_y = 0;
    s.max_abs_vel[0] = 0.0; s.max_abs_vel[1] = 0.0; s.max_abs_u0[0] = 0.0; s.max_abs_u0[1] = 0.0;
    return s;
}
__device__ __forceinline__ void mc_fold_record(ismpc_a_rollout_summary& s, const ismpc_a_out& o, int t)
{
    s.status_or |= o.status;
    if (o.status & ISMPC_A_ST_ERROR_MASK) { if (s.first_error_tick < 0) s.first_error_tick = t; ++s.error_ticks; }
    if (o.status & ISMPC_A_ST_ITER_LIMIT) ++s.iter_limit_ticks;
    s.iters_sum_x += o.iters_x; s.iters_sum_y += o.iters_y;
    s.max_active_x = max(s.max_active_x, o.active & 0xffff); s.max_active_y = max(s.max_active_y, o.active >> 16);
    for (int k = 0; k < 2; ++k) { s.max_abs_vel[k] = fmax(s.max_abs_vel[k], fabs(o.vel_after[k])); s.max_abs_u0[k] = fmax(s.max_abs_u0[k], fabs(o.u0[k])); }
}

// ismpc_a_tick_prologue for tick t of the disturbed loop, in the same single launch: the snapshot, the counters, the PiPre records and
// the cleared flags as there, and per instance (a) the output record of tick t - 1 folded into the summary, (b) the tick's push from
// the instance's table, (c) -- by the host, through `out` -- the trajectory row or the handle's scratch record as the tick's output.
// `out` and mc.last are the same scratch records when neither tick is recorded: the thread that folds a record clears it afterwards.
// A thread per instance reads its n_push table entries 24 n_push bytes apart (uncoalesced; n_push is a handful) and its 80-byte record
// and 64-byte summary as 16-byte words 80 / 64 bytes apart -- a few MB per tick at 16 384 instances, next to a solver launch of milliseconds.
__global__ void ismpc_a_mc_prologue(const ismpc_a_state* __restrict__ state, ismpc_a_state* __restrict__ prev, ismpc_a_out* out, int batch, int* counters,
                                    const ismpc_a_inst* __restrict__ inst, ismpc_a::PiPre* __restrict__ pre, double grav, double dt, int C, int P, McTick mc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 && counters) counters[i] = 0;
    // the snapshot and the PiPre record: ismpc_a_tick_prologue's own statements, kept word for word (that kernel stays as it is)
    {
        constexpr int WPR = (int)(sizeof(ismpc_a_state) / 16);
        const double2* src = reinterpret_cast<const double2*>(state);
        double2* dst = reinterpret_cast<double2*>(prev);
        const long long nw = (long long)batch * WPR;
        for (long long w = i; w < nw; w += (long long)gridDim.x * blockDim.x) dst[w] = src[w];
    }
    if (i >= batch) return;
    if (inst && pre) {
        const double height = inst[i].height;
        const double eta = (height > 0) ? sqrt(grav / height) : 1.0;
        const double lam = exp(-eta * dt);
        auto ipw = [](double b, int n) { double r = 1.0; while (n > 0) { if (n & 1) r *= b; b *= b; n >>= 1; } return r; };
        const double lamC = ipw(lam, C), lamP = ipw(lam, P);
        const double r1 = 1.0 / (1.0 - lam);
        const double k1c = (1 / eta) * (1 - lam) / (1 - lamC), k2c = dt * 1.0 * lamC;
        ismpc_a::PiPre q;
        q.eta = eta; q.lam = lam; q.lamC = lamC; q.lamP = lamP; q.k1c = k1c; q.k2c = k2c;
        q.A1 = k1c * r1; q.A2 = k1c * k1c / ((1.0 - lam) * (1.0 + lam)); q.B2 = 2.0 * k1c * k2c * r1;
        q.aa = (q.A2 * ((1.0 - lamC) * (1.0 + lamC)) - q.B2 * (1.0 - lamC)) + (double)C * (k2c * k2c);
        const double Qf = (inst[i].Qf > 0) ? inst[i].Qf : 1.0;
        const int step = inst[i].step >= 2 ? inst[i].step : 2, ds = inst[i].ds >= 2 ? inst[i].ds : 2;
        q.sqQf = sqrt(Qf); q.isqQf = 1.0 / sqrt(Qf); q.iQf = 1.0 / Qf; q.ieta = 1.0 / eta;
        q.inv_ds = 1.0 / (double)ds; q.inv_dsm1 = 1.0 / (double)(ds - 1); q.rstep = 1.0f / (float)step; q.pad_ = 0;
        const double ie = 1.0 / lam;
        q.ch = 0.5 * (ie + lam); q.sh = 0.5 * (ie - lam); q.sh_eta = q.sh / eta;
        pre[i] = q;
    }
    if (mc.summary) {
        ismpc_a_rollout_summary s = mc_empty_summary();
        if (mc.last) { s = mc.summary[i]; mc_fold_record(s, mc.last[i], mc.t - 1); }
        mc.summary[i] = s;
    }
    if (mc.push) {
        // the prefix-maximum form of the cursor rule: an entry applies when its tick is this one and no earlier entry of the table has a
        // larger tick (ticks outside [0, ticks) are never this one); rebuilt from the table every tick, so no cursor is kept anywhere
        const ismpc_a_push* tab = mc.pushes + (size_t)i * mc.n_push;
        double dx = 0.0, dy = 0.0;
        int top = INT32_MIN;
        for (int k = 0; k < mc.n_push; ++k) {
            const int tk = tab[k].tick;
            if (tk < top) continue;
            top = tk;
            if (tk == mc.t) { dx += tab[k].dv[0]; dy += tab[k].dv[1]; }
        }
        reinterpret_cast<double2*>(mc.push)[i] = make_double2(dx, dy);
    }
    if (out) { out[i].status = 0; out[i].active = 0; out[i].iters_x = 0; out[i].iters_y = 0; }
}

// After the last tick: its output record into the summary (last == NULL: a call of no ticks, the empty summary).
__global__ void ismpc_a_mc_fold(const ismpc_a_out* __restrict__ last, ismpc_a_rollout_summary* __restrict__ summary, int batch, int t)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    ismpc_a_rollout_summary s = mc_empty_summary();
    if (last) { s = summary[i]; mc_fold_record(s, last[i], t); }
    summary[i] = s;
}

}  // namespace

extern "C" {

const char* ismpc_a_last_error(void) { return g_err_a.c_str(); }

void ismpc_a_params_default(int gait, ismpc_a_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    if (gait == 1) { p->C = 100; p->P = 200; p->step = 50; p->ds = 30; p->Qf = 1e9; }     // quad_walk_no_plots.m:20-45,271
    else           { p->C = 160; p->P = 320; p->step = 80; p->ds = 50; p->Qf = 1e7; }     // quad_as_bip_no_plots.m:16-39,257
    p->F = 3; p->n_gait = 100; p->dt = 0.01; p->height = 0.56; p->grav = 9.8; p->w = 0.02;
    p->disp_forw = 0.5; p->disp_forw_dummy = 0.25; p->disp_L = 0.4;
}

void ismpc_a_gait_default(int gait, double phi, double disp_A, ismpc_a_gait* g)
{
    if (!g) return;
    g->gait = gait; g->n_gait = 100; g->disp_A = disp_A; g->phi = phi;
    g->disp_B = 0.259394; g->disp_C = 0.88; g->disp_i = 0.4; g->disp_o = 0.4; g->disp_forw = 0.5;
}

// The step and the first (half) step of a plan, clipped to the kinematic limits (init_quadruped*.m:55-102): everything in a plan that
// takes cos, sin or atan.  ismpc_a_plan and ismpc_a_create_plans (whose generator kernel gets these four doubles per plan) share it.
int ismpc_a_plan_steps(const ismpc_a_gait* g, double steps[4])
{
    if (!g || !steps) return fail_a(-1, "ismpc_a_plan_steps: null argument");
    const double dfd = g->disp_forw / 2, dv = std::min(g->disp_i, g->disp_o), dvd = dv / 2;
    double xs = g->disp_A * std::cos(g->phi), ys = g->disp_A * std::sin(g->phi);
    double xsd = g->disp_A * std::cos(g->phi) / 2, ysd = g->disp_A * std::sin(g->phi) / 2;
    int branches = 0;
    auto clip = [&](double& x, double& y, double vlim, double flim, int bit) {
        if (y > vlim || x > flim) {
            if (g->phi > std::atan(vlim / flim)) { y = vlim; x = vlim * std::cos(g->phi) / std::sin(g->phi); branches |= bit; }
            else { x = flim; y = flim * std::sin(g->phi) / std::cos(g->phi); branches |= 2 * bit; }
        }
    };
    clip(xsd, ysd, dvd, dfd, 1);          // first (half) step   :62-81
    clip(xs, ys, dv, g->disp_forw, 4);    // regular step        :84-102
    steps[0] = xs; steps[1] = ys; steps[2] = xsd; steps[3] = ysd;
    return branches;
}

// trotting/init_quadruped.m:5-184, walking/init_quadruped2.m:5-284 (host; once per run)
int ismpc_a_plan(const ismpc_a_gait* g, double* foot_plan, double* center)
{
    if (!g || !foot_plan || !center || g->n_gait < 16) return fail_a(-1, "bad argument");
    const int NG = g->n_gait;
    double steps[4];
    ismpc_a_plan_steps(g, steps);
    const double xs = steps[0], ys = steps[1], xsd = steps[2], ysd = steps[3];
    const int rows = NG + 1;           // 1-based rows 1..NG+1 stored at index row-1
    std::vector<double> fp((size_t)(rows + 8) * 8);
    auto FP = [&](int r, int col) -> double& { return fp[(size_t)(r - 1) * 8 + (col - 1)]; };
    for (int r = 1; r <= rows + 7; ++r) {
        FP(r,1) = 0.0; FP(r,2) = g->disp_B; FP(r,3) = 0.0; FP(r,4) = -g->disp_B;
        FP(r,5) = g->disp_C; FP(r,6) = -g->disp_B; FP(r,7) = g->disp_C; FP(r,8) = g->disp_B;
    }
    auto cross = [&](int r, double& cx, double& cy) {      // intersection of the diagonals BL-FR and BR-FL
        const double m1 = (FP(r,6) - FP(r,2)) / (FP(r,5) - FP(r,1)), b1 = FP(r,2) - m1 * FP(r,1);
        const double m2 = (FP(r,8) - FP(r,4)) / (FP(r,7) - FP(r,3)), b2 = FP(r,4) - m2 * FP(r,3);
        cx = (b2 - b1) / (m1 - m2); cy = m1 * cx + b1;
    };
    for (int r = 0; r < NG; ++r) { center[r * 2] = 0.0; center[r * 2 + 1] = 0.0; }
    center[0] = g->disp_C / 2;
    int used = NG;
    if (g->gait == 0) {
        FP(2,1) = xsd; FP(2,5) = g->disp_C + xsd; FP(2,2) = g->disp_B + ysd; FP(2,6) = -g->disp_B + ysd;
        for (int j = 3; j <= NG; ++j) {
            const bool even = (j % 2) == 0;
            const int mv1 = even ? 1 : 3, mv2 = even ? 5 : 7, hd1 = even ? 3 : 1, hd2 = even ? 7 : 5;
            FP(j, mv1) = FP(j-1, mv1) + xs; FP(j, mv2) = FP(j-1, mv2) + xs; FP(j, hd1) = FP(j-1, hd1); FP(j, hd2) = FP(j-1, hd2);
            FP(j, mv1+1) = FP(j-1, mv1+1) + ys; FP(j, mv2+1) = FP(j-1, mv2+1) + ys; FP(j, hd1+1) = FP(j-1, hd1+1); FP(j, hd2+1) = FP(j-1, hd2+1);
        }
        for (int k = 2; k <= NG; ++k) cross(k, center[(k-1)*2], center[(k-1)*2+1]);
    } else {
        FP(3,7) = g->disp_C + xsd; FP(4,7) = FP(3,7); FP(5,7) = FP(3,7);
        FP(2,3) = FP(1,3); FP(3,3) = FP(1,3); FP(4,3) = FP(3,3); FP(5,3) = FP(4,3) + xsd;
        FP(3,8) = g->disp_B + ysd; FP(4,8) = FP(3,8); FP(5,8) = FP(3,8);
        FP(2,4) = FP(1,4); FP(3,4) = FP(1,4); FP(4,4) = FP(3,4); FP(5,4) = FP(4,4) + ysd;
        for (int j = 6; j <= NG; j += 8) {
            for (int cc = 0; cc < 2; ++cc) {
                const double st = cc == 0 ? xs : ys;
                const int BL = 1 + cc, BR = 3 + cc, FR = 5 + cc, FL = 7 + cc;
                FP(j,FR) = FP(j-1,FR); FP(j+1,FR) = FP(j,FR) + st; for (int k = 2; k <= 7; ++k) FP(j+k,FR) = FP(j+1,FR);
                FP(j,BL) = FP(j-1,BL); FP(j+1,BL) = FP(j,BL); FP(j+2,BL) = FP(j,BL); FP(j+3,BL) = FP(j+2,BL) + st;
                for (int k = 4; k <= 7; ++k) FP(j+k,BL) = FP(j+3,BL);
                FP(j,FL) = FP(j-1,FL); for (int k = 1; k <= 4; ++k) FP(j+k,FL) = FP(j,FL);
                FP(j+5,FL) = FP(j+4,FL) + st; FP(j+6,FL) = FP(j+5,FL); FP(j+7,FL) = FP(j+5,FL);
                FP(j,BR) = FP(j-1,BR); for (int k = 1; k <= 6; ++k) FP(j+k,BR) = FP(j,BR);
                FP(j+7,BR) = FP(j+6,BR) + st;
            }
            used = std::max(used, j + 7);
        }
        used = std::min(used, NG + 1);
        // (for some NG, 23 among them, the script's array grows past row NG; the caller's `center` has NG rows: those rows are not written)
        for (int j = 1; j <= NG - 4; j += 8) {
            for (int k = 0; k <= 6; k += 2) if (j + k <= NG) cross(j + k, center[(j+k-1)*2], center[(j+k-1)*2+1]);
            for (int k = 1; k <= 7; k += 2) if (j + k <= NG) { center[(j+k-1)*2] = center[(j+k-2)*2]; center[(j+k-1)*2+1] = center[(j+k-2)*2+1]; }
        }
    }
    std::memcpy(foot_plan, fp.data(), sizeof(double) * (size_t)used * 8);
    return used;
}

int ismpc_a_create(const ismpc_a_params* p, const double* center, int device, ismpc_a_handle** out)
{
    if (!p || !center || !out) return fail_a(-1, "null argument");
    *out = nullptr;
    if (p->C < 2 || p->F < 1 || p->F > MAXF || p->C + p->F > T || p->P <= p->C || p->step < 2 || p->ds < 2 || p->ds >= p->step ||
        p->n_gait < p->F + 2 || !(p->dt > 0) || !(p->height > 0) || !(p->Qf > 0) || !(p->w >= 0))
        return fail_a(-1, "unsupported parameters (need 2 <= C, C + F <= 256, 1 <= F <= 8, P > C, 2 <= ds < step)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail_a(-2, "no HIP device visible: the ISMPC hot path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail_a(-1, "device ordinal out of range");
    ismpc_a_handle* h = new (std::nothrow) ismpc_a_handle();
    if (!h) return fail_a(-3, "out of host memory");
    h->p = *p; h->device = device;
    DeviceGuardA guard_(device);
    if (guard_.err != hipSuccess) { delete h; return fail_a(-2, "hipSetDevice failed"); }
    DevA& c = h->c;
    c.C = p->C; c.P = p->P; c.F = p->F; c.step = p->step; c.ds = p->ds; c.n_gait = p->n_gait;
    c.dt = p->dt; c.eta = std::sqrt(p->grav / p->height); c.w = p->w; c.Qf = p->Qf;
    c.disp_forw = p->disp_forw; c.disp_forw_dummy = p->disp_forw_dummy; c.disp_L = p->disp_L;
    c.ldq = (p->C + p->F + 2) | 1;                        // odd leading dimension: conflict-free LDS columns
    c.max_iter = 20 * (p->C + p->F) + 200;
    env_switch("ISMPC_A_HISTORY", false, &h->hist_off);          // =0: no working-set history
    env_switch("ISMPC_A_BUCKET", true, &h->bucket_by_F);
    if (env_is("ISMPC_A_PRECISION", "f32") && p->F >= 3 && p->F <= 6) h->precision = 1;   // A/B knob
    if (env_is("ISMPC_A_KERNEL", "block")) h->use_wave = false;
    // ISMPC_A_WARM=add,drop,extra,min_viol,gi_first,peel,rounds,round_adds overrides; ISMPC_A_WARM=0 starts every QP cold
    c.warm_add = 8; c.warm_drop = 12; c.warm_extra = 0; c.warm_min_viol = 6; c.warm_gi = 2; c.warm_peel_end = 1;
    c.warm_rounds = 2; c.warm_round_adds = 8;
    env_switch("ISMPC_A_F32_RESOLVE", false, &h->defer_off);
    env_int("ISMPC_A_RESOLVE_GRID", 1, 1024, &h->resolve_grid);
    env_int("ISMPC_A_STATIC", 0, 16, &h->static_q);
    env_int("ISMPC_A_CLAIM", 0, 64, &h->claim_chunk);             // 0: by shape
    if (const char* e = std::getenv("ISMPC_A_WARM")) {
        int a_ = 0, d_ = 0, x_ = 0, v_ = 0, g_ = 0, pe_ = 0, r_ = 0, ra_ = 0;
        const int got = std::sscanf(e, "%d,%d,%d,%d,%d,%d,%d,%d", &a_, &d_, &x_, &v_, &g_, &pe_, &r_, &ra_);
        if (got >= 1) c.warm_add = clampi(a_, 0, 32);
        if (got >= 2) c.warm_drop = clampi(d_, 0, 32);
        if (got >= 3) c.warm_extra = clampi(x_, 0, 8);
        if (got >= 4) c.warm_min_viol = clampi(v_, 1, 256);
        if (got >= 5) c.warm_gi = clampi(g_, 0, 64);
        if (got >= 6) c.warm_peel_end = pe_ != 0;
        if (got >= 7) c.warm_rounds = clampi(r_, 0, 16);
        if (got >= 8) c.warm_round_adds = clampi(ra_, 1, 64);
    }
    // S^-1 lives in an L2-resident scratch slab (4 workgroups per CU); ISMPC_A_SINV=lds keeps it in LDS instead when it
    // fits next to the static block (then 1 workgroup per CU).  Measured on MI355X (walk, C=100, batch 16 384):
    // scratch 2.8e5 ticks/s, LDS 2.0e5 ticks/s -- the kernel is barrier-latency bound, concurrency wins.
    c.sinv_in_lds = 0;
    if (env_is("ISMPC_A_SINV", "lds") && (size_t)c.ldq * c.ldq * sizeof(double) + sizeof(Shared) + 1024 <= 160u * 1024u) c.sinv_in_lds = 1;
    const double eta = c.eta, dt = c.dt;
    const double ch = std::cosh(eta * dt), sh = std::sinh(eta * dt);                           // :67-71
    const double Au[9] = { ch, sh / eta, 1 - ch, eta * sh, ch, -eta * sh, 0, 0, 1 };
    const double Bu[3] = { dt - sh / eta, 1 - ch, dt };
    std::memcpy(c.Au, Au, sizeof(Au)); std::memcpy(c.Bu, Bu, sizeof(Bu));
    // stability row (:233-238) and tail weights (:229-231)
    const double lambda = std::exp(-eta * dt);
    std::vector<double> a(p->C), PA(p->C + 1, 0.0), PA2(p->C + 1, 0.0), wt(p->P - p->C);
    double aa = 0.0;
    for (int i = 0; i < p->C; ++i) {
        a[i] = (1 / eta) * (1 - lambda) / (1 - std::pow(lambda, p->C)) * std::exp(-eta * dt * i) - dt * 1.0 * std::exp(-eta * dt * p->C);
        PA[i + 1] = PA[i] + a[i]; aa += a[i] * a[i]; PA2[i + 1] = aa;
    }
    double sumw = 0.0;
    for (int i = p->C + 1; i <= p->P; ++i) { wt[i - (p->C + 1)] = std::exp(-eta * dt * i) * (1 - std::exp(-eta * dt)); sumw += wt[i - (p->C + 1)]; }
    c.wP = std::exp(-eta * dt * p->P); c.sumw = sumw + c.wP; c.aa = aa;
    c.sqQf = std::sqrt(c.Qf); c.isqQf = 1.0 / std::sqrt(c.Qf); c.iQf = 1.0 / c.Qf; c.ieta = 1.0 / eta;
    c.inv_ds = 1.0 / (double)p->ds; c.rstep = 1.0f / (float)p->step;
    h->fsx.resize(p->n_gait); h->fsy.resize(p->n_gait);
    for (int i = 0; i < p->n_gait; ++i) { h->fsx[i] = center[i * 2]; h->fsy[i] = center[i * 2 + 1]; }
    std::vector<double> clx0, cly0, clx1, cly1;
    centreline(h->fsx, p->step, p->ds, p->n_gait, true, clx0);  centreline(h->fsy, p->step, p->ds, p->n_gait, true, cly0);
    centreline(h->fsx, p->step, p->ds, p->n_gait, false, clx1); centreline(h->fsy, p->step, p->ds, p->n_gait, false, cly1);
    c.ncl = (int)std::min(clx0.size(), clx1.size());
    int rc = upload_a(h, a, &c.a);
    if (!rc) rc = upload_a(h, PA, &c.PA);
    if (!rc) rc = upload_a(h, PA2, &c.PA2);
    if (!rc) rc = upload_a(h, wt, &c.wtail);
    if (!rc) rc = upload_a(h, h->fsx, &c.fsx);
    if (!rc) rc = upload_a(h, h->fsy, &c.fsy);
    if (!rc) {
        // the centres of the base plans per-instance launches choose from: four slots of n_gait x values, then four of n_gait y values
        std::vector<double> tab((size_t)8 * p->n_gait, 0.0);
        std::copy(h->fsx.begin(), h->fsx.end(), tab.begin());
        std::copy(h->fsy.begin(), h->fsy.end(), tab.begin() + (size_t)4 * p->n_gait);
        const double* t0 = nullptr;
        rc = upload_a(h, tab, &t0);
        if (!rc) { h->plan_tab = const_cast<double*>(t0); c.tab_x = t0; c.tab_y = t0 + (size_t)4 * p->n_gait; c.nplans = 1; c.grav = p->grav; }
    }
    if (!rc) rc = upload_a(h, clx0, &c.clx0);
    if (!rc) rc = upload_a(h, cly0, &c.cly0);
    if (!rc) rc = upload_a(h, clx1, &c.clx1);
    if (!rc) rc = upload_a(h, cly1, &c.cly1);
    // the tail sums of the wave kernel, one per tick index and centreline table (long double: they replace a 64-lane fp64 reduction)
    auto tail_table = [&](const std::vector<double>& cl, const double** dst) -> int {
        const int nt = c.ncl - p->P + 1;
        std::vector<double> T(std::max(nt, 1), 0.0);
        for (int j = 0; j < nt; ++j) {
            long double s = 0.0L;
            for (int i = p->C + 1; i <= p->P; ++i) s += (long double)wt[i - (p->C + 1)] * (long double)cl[j + i - 1];
            T[j] = (double)(s + (long double)c.wP * (long double)cl[p->P - 1]);
        }
        return upload_a(h, T, dst);
    };
    if (!rc) rc = tail_table(clx0, &c.tlx0);
    if (!rc) rc = tail_table(cly0, &c.tly0);
    if (!rc) rc = tail_table(clx1, &c.tlx1);
    if (!rc) rc = tail_table(cly1, &c.tly1);
    if (!rc) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess) rc = fail_a(-2, "hipGetDeviceProperties failed");
        else {
            h->slots = prop.multiProcessorCount * (c.sinv_in_lds ? 1 : 4);   // persistent grid: workgroups per CU
            const int scratch_slots = prop.multiProcessorCount * 4;          // the slab always covers the 4-per-CU grid (the LDS variant may fall back to it)
            h->wave_blocks = prop.multiProcessorCount * 4; h->cus = prop.multiProcessorCount;
            if (hipMalloc((void**)&h->work_counter, 4 * sizeof(int)) != hipSuccess) rc = fail_a(-3, "counter allocation failed");
            else h->allocs.push_back(h->work_counter);
            if (!rc) { if (hipMalloc((void**)&h->c_dev, sizeof(DevA)) != hipSuccess) rc = fail_a(-3, "constants allocation failed"); else h->allocs.push_back(h->c_dev); }
            void* sc = nullptr;
            if (hipMalloc(&sc, (size_t)scratch_slots * c.ldq * c.ldq * sizeof(double)) != hipSuccess) rc = fail_a(-3, "scratch allocation failed");
            else { h->allocs.push_back(sc); c.scratch = static_cast<double*>(sc); }
        }
    }
    if (!rc && c.sinv_in_lds) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(ismpc_a_tick_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((size_t)c.ldq * c.ldq * sizeof(double))) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(ismpc_a_tick_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((size_t)c.ldq * c.ldq * sizeof(double))) != hipSuccess) c.sinv_in_lds = 0, h->slots *= 4;
    }
    if (!rc && hipMemcpy(h->c_dev, &h->c, sizeof(DevA), hipMemcpyHostToDevice) != hipSuccess) rc = fail_a(-2, "constants upload failed");
    if (rc) { ismpc_a_destroy(h); return rc; }
    h->c_dirty = false;
    *out = h;
    return 0;
}

void ismpc_a_destroy(ismpc_a_handle* h)
{
    if (!h) return;
    DeviceGuardA guard_(h->device);
    for (void* p : h->allocs) (void)hipFree(p);
    for (void* p : h->scratch()) if (p) (void)hipFree(p);
    delete h;
}

int ismpc_a_initial_state(const ismpc_a_handle* h, double disp_C, ismpc_a_state* st)
{
    if (!h || !st) return fail_a(-1, "null argument");
    std::memset(st, 0, sizeof(*st));
    st->x = disp_C / 2; st->xz = disp_C / 2;                  // :52-57
    st->cur_x = h->fsx[0]; st->cur_y = h->fsy[0];             // :58-59
    st->fc = 1; st->j = 1;
    return 0;
}

int ismpc_a_add_plan(ismpc_a_handle* h, const double* center)
{
    if (!h || !center) return fail_a(-1, "null argument");
    if (h->table) return fail_a(-1, "ismpc_a_add_plan: the plans of a plan-table handle are those given to ismpc_a_create_plans");
    if (h->c.nplans >= 4) return fail_a(-1, "at most 4 base plans per handle");
    ON_DEVICE_A(h);
    const int NG = h->p.n_gait;
    std::vector<double> px(NG), py(NG);
    for (int i = 0; i < NG; ++i) { px[i] = center[i * 2]; py[i] = center[i * 2 + 1]; }
    const int k = h->c.nplans;
    HIP_TRY_A(hipMemcpy(h->plan_tab + (size_t)k * NG, px.data(), sizeof(double) * NG, hipMemcpyHostToDevice));
    HIP_TRY_A(hipMemcpy(h->plan_tab + (size_t)(4 + k) * NG, py.data(), sizeof(double) * NG, hipMemcpyHostToDevice));
    h->c.nplans = k + 1;
    HIP_TRY_A(hipMemcpy(h->c_dev, &h->c, sizeof(DevA), hipMemcpyHostToDevice));
    return k;
}

// ---- plan-table handles
namespace {
struct DevTemp { void* p = nullptr; ~DevTemp() { if (p) (void)hipFree(p); } };   // device memory of one call

// All plans of `gaits` into one table on the handle's device (the current one), by one launch of ismpc_a_plan_table_kernel.
int build_plan_table(ismpc_a_handle* h, const ismpc_a_gait* gaits, int n_plans)
{
    const int NG = h->p.n_gait, FR = plan_table_rows(NG);
    std::vector<double> steps((size_t)n_plans * 4);
    for (int k = 0; k < n_plans; ++k) ismpc_a_plan_steps(&gaits[k], &steps[(size_t)k * 4]);
    h->gaits.assign(gaits, gaits + n_plans);
    void *centres = nullptr, *feet = nullptr, *rules = nullptr;
    HIP_TRY_A(hipMalloc(&centres, sizeof(double) * 2 * (size_t)n_plans * NG)); h->allocs.push_back(centres);
    HIP_TRY_A(hipMalloc(&feet, sizeof(double) * 8 * (size_t)n_plans * FR)); h->allocs.push_back(feet);
    HIP_TRY_A(hipMalloc(&rules, sizeof(FeetParams) * (size_t)n_plans)); h->allocs.push_back(rules);
    DevTemp g_dev, s_dev;
    HIP_TRY_A(hipMalloc(&g_dev.p, sizeof(ismpc_a_gait) * (size_t)n_plans));
    HIP_TRY_A(hipMalloc(&s_dev.p, sizeof(double) * 4 * (size_t)n_plans));
    HIP_TRY_A(hipMemcpy(g_dev.p, gaits, sizeof(ismpc_a_gait) * (size_t)n_plans, hipMemcpyHostToDevice));
    HIP_TRY_A(hipMemcpy(s_dev.p, steps.data(), sizeof(double) * 4 * (size_t)n_plans, hipMemcpyHostToDevice));
    double* tx = static_cast<double*>(centres);
    double* ty = tx + (size_t)n_plans * NG;
    hipEvent_t e0 = nullptr, e1 = nullptr;                         // the launch's own time (ismpc_a_plans_build_ms)
    HIP_TRY_A(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return fail_a(-2, "hipEventCreate failed"); }
    (void)hipEventRecord(e0, nullptr);
    const unsigned grid = (unsigned)(((size_t)n_plans * 8 + PLAN_GEN_THREADS - 1) / PLAN_GEN_THREADS);
    hipLaunchKernelGGL(ismpc_a_plan_table_kernel, dim3(grid), dim3(PLAN_GEN_THREADS), 0, nullptr, (const ismpc_a_gait*)g_dev.p, (const double*)s_dev.p,
                       n_plans, NG, tx, ty, static_cast<double*>(feet), static_cast<FeetParams*>(rules));
    hipError_t err = hipGetLastError();
    (void)hipEventRecord(e1, nullptr);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail_a(-2, std::string("ismpc_a_plan_table_kernel: ") + hipGetErrorString(err));
    h->build_ms = ms;
    h->table = true; h->tab_feet = static_cast<double*>(feet); h->tab_rules = static_cast<FeetParams*>(rules);
    h->c.tab_x = tx; h->c.tab_y = ty; h->c.nplans = n_plans;
    HIP_TRY_A(hipMemcpy(h->c_dev, &h->c, sizeof(DevA), hipMemcpyHostToDevice));
    return 0;
}
}  // namespace

int ismpc_a_create_plans(const ismpc_a_params* p, const ismpc_a_gait* gaits, int n_plans, int device, ismpc_a_handle** out)
{
    if (!p) return fail_a(-1, "ismpc_a_create_plans: null params");
    if (!gaits) return fail_a(-1, "ismpc_a_create_plans: null gaits");
    if (!out) return fail_a(-1, "ismpc_a_create_plans: null out");
    *out = nullptr;
    if (n_plans < 1) return fail_a(-1, "ismpc_a_create_plans: n_plans must be at least 1");
    if (n_plans > ISMPC_A_MAX_PLANS) return fail_a(-1, "ismpc_a_create_plans: n_plans beyond ISMPC_A_MAX_PLANS");
    if (p->n_gait < 16) return fail_a(-1, "ismpc_a_create_plans: n_gait must be at least 16");
    for (int k = 0; k < n_plans; ++k) {
        if (gaits[k].n_gait != p->n_gait) return fail_a(-1, "ismpc_a_create_plans: n_gait of gaits[" + std::to_string(k) + "] differs from the parameters'");
        if (gaits[k].gait != 0 && gaits[k].gait != 1) return fail_a(-1, "ismpc_a_create_plans: gait of gaits[" + std::to_string(k) + "] is neither 0 (trot) nor 1 (walk)");
    }
    try {
        // plan 0 on the host: what the plain launches, the centreline tables and the tails are built from, as ismpc_a_create does
        std::vector<double> fp0((size_t)(p->n_gait + 1) * 8), ce0((size_t)p->n_gait * 2);
        if (ismpc_a_plan(&gaits[0], fp0.data(), ce0.data()) < 0) return -1;
        ismpc_a_handle* h = nullptr;
        if (int rc = ismpc_a_create(p, ce0.data(), device, &h)) return rc;
        int rc;
        {
            DeviceGuardA guard_(device);
            rc = guard_.err != hipSuccess ? fail_a(-2, "hipSetDevice failed") : build_plan_table(h, gaits, n_plans);
        }
        if (rc) { ismpc_a_destroy(h); return rc; }
        *out = h;
    } catch (const std::bad_alloc&) {
        return fail_a(-3, "ismpc_a_create_plans: out of host memory");
    }
    return 0;
}

int ismpc_a_plans_info(const ismpc_a_handle* h, int* n_plans)
{
    if (!h || !n_plans) return fail_a(-1, "ismpc_a_plans_info: null argument");
    *n_plans = h->c.nplans;
    return 0;
}

double ismpc_a_plans_build_ms(const ismpc_a_handle* h) { return (h && h->table) ? (double)h->build_ms : -1.0; }

int ismpc_a_get_plan(ismpc_a_handle* h, int plan, double* foot_plan, double* center)
{
    if (!h) return fail_a(-1, "ismpc_a_get_plan: null handle");
    if (!h->table) return fail_a(-1, "ismpc_a_get_plan: needs a handle of ismpc_a_create_plans");
    if (plan < 0 || plan >= h->c.nplans) return fail_a(-1, "ismpc_a_get_plan: plan index out of range");
    ON_DEVICE_A(h);
    const int NG = h->p.n_gait, used = plan_used_rows(h->gaits[plan].gait, NG);
    if (foot_plan) HIP_TRY_A(hipMemcpy(foot_plan, h->tab_feet + (size_t)plan * plan_table_rows(NG) * 8, sizeof(double) * 8 * (size_t)used, hipMemcpyDeviceToHost));
    if (center) {
        std::vector<double> x(NG), y(NG);
        HIP_TRY_A(hipMemcpy(x.data(), h->c.tab_x + (size_t)plan * NG, sizeof(double) * NG, hipMemcpyDeviceToHost));
        HIP_TRY_A(hipMemcpy(y.data(), h->c.tab_y + (size_t)plan * NG, sizeof(double) * NG, hipMemcpyDeviceToHost));
        for (int i = 0; i < NG; ++i) { center[i * 2] = x[i]; center[i * 2 + 1] = y[i]; }
    }
    return used;
}

int ismpc_a_initial_state_plan(const ismpc_a_handle* h, int plan, ismpc_a_state* st)
{
    if (!h || !st) return fail_a(-1, "ismpc_a_initial_state_plan: null argument");
    if (!h->table) return fail_a(-1, "ismpc_a_initial_state_plan: needs a handle of ismpc_a_create_plans");
    if (plan < 0 || plan >= h->c.nplans) return fail_a(-1, "ismpc_a_initial_state_plan: plan index out of range");
    ON_DEVICE_A(h);
    double f0[2];
    HIP_TRY_A(hipMemcpy(&f0[0], h->c.tab_x + (size_t)plan * h->p.n_gait, sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY_A(hipMemcpy(&f0[1], h->c.tab_y + (size_t)plan * h->p.n_gait, sizeof(double), hipMemcpyDeviceToHost));
    std::memset(st, 0, sizeof(*st));
    const double disp_C = h->gaits[plan].disp_C;
    st->x = disp_C / 2; st->xz = disp_C / 2;                  // :52-57
    st->cur_x = f0[0]; st->cur_y = f0[1];                     // :58-59
    st->fc = 1; st->j = 1;
    return 0;
}

int ismpc_a_reserve(ismpc_a_handle* h, int max_batch)
{
    if (!h || max_batch < 0) return fail_a(-1, "bad argument");
    ON_DEVICE_A(h);
    if (max_batch > h->prev_cap) ISMPC_GROW_SYNC(fail_a, h->prev, h->prev_cap, max_batch, sizeof(ismpc_a_state) * (size_t)max_batch);
    if (max_batch > h->order_cap) ISMPC_GROW_SYNC(fail_a, h->order, h->order_cap, max_batch, sizeof(int) * (4 * (size_t)max_batch + 4));
    if (max_batch > h->pre_cap) ISMPC_GROW_SYNC(fail_a, h->pre, h->pre_cap, max_batch, sizeof(ismpc_a::PiPre) * (size_t)max_batch);
    if (max_batch > h->defer_cap) ISMPC_GROW_SYNC(fail_a, h->defer_list, h->defer_cap, max_batch, sizeof(int) * 2 * (size_t)max_batch);
    if (max_batch > h->hist_cap) {
        h->hist_valid = false;
        ISMPC_GROW_SYNC(fail_a, h->hist, h->hist_cap, max_batch, sizeof(unsigned long long) * 16 * (size_t)max_batch);
    }
    if (max_batch > h->mc_cap) ISMPC_GROW_SYNC(fail_a, h->mc, h->mc_cap, max_batch, MC_BYTES_PER_INSTANCE * (size_t)max_batch);
    return 0;
}

// The handle's scratch (prev, pre, hist, order, defer_list) outlives the call that allocated it and is used by later calls on
// whatever stream those pass: it grows through ISMPC_GROW_ASYNC (ismpc_host.hpp), which drains the previous launch's stream first.
static int tick_launch(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, const double* push_dev,
                       ismpc_a_out* out_dev, void* stream, int history = -1, const McTick* mc = nullptr, double* dec_dev = nullptr)
{
    // mc: a tick of the disturbed closed loop (rollout_mc_a): its prologue in place of the plain one, everything else as always
    // dec_dev: the solver launch(es) run in the form that also stores every QP's whole decision there (ismpc_a_tick_batch_horizon_device)
    if (!h || batch < 0 || (batch > 0 && !state_dev)) return fail_a(-1, "bad argument");
    if (batch == 0) return 0;
    ON_DEVICE_A(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // history: -1 = as set by ismpc_a_set_warm_history, 0 = none, 1 = first tick of a rollout (store only), 2 = load + store
    if (history < 0) history = h->hist_ticks ? ((h->hist_valid && h->hist_batch == batch) ? 2 : 1) : 0;
    if (h->c.warm_add <= 0 || h->hist_off) history = 0;
    unsigned long long* hist = nullptr;
    if (history > 0) {
        if (batch > h->hist_cap) {                       // stream-ordered growth; ismpc_a_reserve sizes it beforehand
            h->hist_valid = false;
            ISMPC_GROW_ASYNC(fail_a, h, h->hist, h->hist_cap, batch, sizeof(unsigned long long) * 16 * (size_t)batch, s);
        }
        hist = h->hist;
        if (history == 2 && !(h->hist_valid && h->hist_batch == batch)) history = 1;
        h->hist_valid = true; h->hist_batch = batch;
    }
    const int hist_load = history == 2 ? 1 : 0;
    ismpc_host::StreamMark<ismpc_a_handle> mark_{h, s};
    if (batch > h->prev_cap) {
        ISMPC_GROW_ASYNC(fail_a, h, h->prev, h->prev_cap, batch, sizeof(ismpc_a_state) * (size_t)batch, s);
    }
    if (inst_dev && batch > h->pre_cap) {
        ISMPC_GROW_ASYNC(fail_a, h, h->pre, h->pre_cap, batch, sizeof(ismpc_a::PiPre) * (size_t)batch, s);
    }
    int* const counters = (h->use_wave || inst_dev) ? h->work_counter : nullptr;
    ismpc_a::PiPre* const pre = inst_dev ? h->pre : nullptr;
    if (mc) {
        hipLaunchKernelGGL(ismpc_a_mc_prologue, dim3((batch + 255) / 256), dim3(256), 0, s, (const ismpc_a_state*)state_dev, h->prev, out_dev, batch,
                           counters, inst_dev, pre, h->c.grav, h->c.dt, h->c.C, h->c.P, *mc);
    } else {
        hipLaunchKernelGGL(ismpc_a_tick_prologue, dim3((batch + 255) / 256), dim3(256), 0, s, (const ismpc_a_state*)state_dev, h->prev, out_dev, batch,
                           counters, inst_dev, pre, h->c.grav, h->c.dt, h->c.C, h->c.P);
    }
    if (h->use_wave || inst_dev) {
        // structured solver, one wavefront per QP, 4 per workgroup; persistent grid (ismpc_a_wave.hpp)
        const int rl = (h->c.C + 63) / 64;
        if (h->c_dirty) { HIP_TRY_A(hipMemcpyAsync(h->c_dev, &h->c, sizeof(DevA), hipMemcpyHostToDevice, s)); h->c_dirty = false; }
        ismpc_a::WaveLaunch WL{h->c_dev, h->c.F, h->prev, state_dev, inst_dev, push_dev, out_dev, batch, h->work_counter, hist, hist_load,
                               h->precision, h->cus, h->wave_occ, nullptr, nullptr, 1, 0, 0, nullptr, nullptr, 0, s};
        // QPs per work-counter atomic (scripts/claim_sweep.sh): one device-wide atomic per QP costs 10-50 % when QPs are short (two rows
        // per lane, the fp32 solve at three, closed-loop ticks); pairs coarsen the balance too much when they are long
        WL.static_q = h->static_q; WL.pre = inst_dev ? h->pre : nullptr; WL.dec = dec_dev;
        WL.claim_chunk = h->claim_chunk > 0 ? h->claim_chunk : ((rl <= 2 || (h->precision == 1 && rl == 3) || hist_load) ? 2 : 1);
        hipError_t werr = hipSuccess;
        int wrc = -1;
        auto go = [&](const ismpc_a::WaveLaunch& W) {
            switch (rl) {
                case 1: case 2: return W.dec ? ismpc_a::launch_wave_rl2_hz(W, &werr) : ismpc_a::launch_wave_rl2(W, &werr);
                case 3: return W.dec ? ismpc_a::launch_wave_rl3_hz(W, &werr) : ismpc_a::launch_wave_rl3(W, &werr);
                case 4: return W.dec ? ismpc_a::launch_wave_rl4_hz(W, &werr) : ismpc_a::launch_wave_rl4(W, &werr);
                default: return -1;
            }
        };
        if (inst_dev && h->c.F > 3 && h->bucket_by_F && rl <= 4 && h->c.F <= 6) {
            if (batch > h->order_cap) {
                ISMPC_GROW_ASYNC(fail_a, h, h->order, h->order_cap, batch, sizeof(int) * (4 * (size_t)batch + 4), s);
            }
            int* counts = h->order + 4 * (size_t)h->order_cap;
            HIP_TRY_A(hipMemsetAsync(counts, 0, 4 * sizeof(int), s));
            hipLaunchKernelGGL(ismpc_a_bucket_by_F, dim3((batch + 255) / 256), dim3(256), 0, s, inst_dev, batch, h->c.F, h->order, h->order_cap, counts);
            wrc = 0;
            for (int f = 3; f <= h->c.F && wrc == 0; ++f) {
                if (f > 3) HIP_TRY_A(hipMemsetAsync(h->work_counter, 0, sizeof(int), s));
                ismpc_a::WaveLaunch W = WL;
                W.F = f; W.order = h->order + (size_t)(f - 3) * h->order_cap; W.count_ptr = counts + (f - 3);
                wrc = go(W);
            }
        } else {
            const bool resolve = h->precision == 1 && !h->defer_off;
            if (resolve) {
                if (batch > h->defer_cap) {                  // stream-ordered growth, as the history
                    ISMPC_GROW_ASYNC(fail_a, h, h->defer_list, h->defer_cap, batch, sizeof(int) * 2 * (size_t)batch, s);
                }
                WL.defer_list = h->defer_list; WL.defer_count = h->work_counter + 2;
            }
            wrc = go(WL);
            if (wrc == 0 && resolve) {
                // the QPs the fp32 launch handed over (block-solve check failed: a horizon pinned end to end), solved by the fp64
                // instantiation: usually nothing to do
                ismpc_a::WaveLaunch W2 = WL;
                W2.precision = 0; W2.work_counter = h->work_counter + 1; W2.order = h->defer_list; W2.count_ptr = h->work_counter + 2;
                W2.order_is_qp = 1; W2.defer_list = nullptr; W2.defer_count = nullptr; W2.static_q = 0; W2.claim_chunk = 1;
                // usually nothing to do (one QP in 30 000 on the bench pushes), but harder pushes hand over hundreds: up to 64 workgroups
                // (256 QPs at a time); a workgroup that finds the list empty exits after its prologue
                W2.grid_cap = h->resolve_grid;
                wrc = go(W2);
            }
        }
        if (wrc == 0) return 0;
        if (wrc == -2) return fail_a(-2, std::string("wave kernel launch: ") + hipGetErrorString(werr));
        if (inst_dev) return fail_a(-1, "per-instance gait parameters need the structured kernel: 3 <= F <= 6 and C <= 256");
        if (h->precision != 0) return fail_a(-1, "the fp32 solve needs the structured kernel: 3 <= F <= 6 and C <= 256");
    }
    const int grid = std::min(2 * batch, h->slots);
    const size_t sinv_bytes = h->c.sinv_in_lds ? (size_t)h->c.ldq * h->c.ldq * sizeof(double) : 0;
    if (dec_dev) hipLaunchKernelGGL(ismpc_a_tick_kernel<true>, dim3(grid), dim3(T), sinv_bytes, s, h->c, (const ismpc_a_state*)h->prev, state_dev, push_dev, out_dev, batch, dec_dev);
    else hipLaunchKernelGGL(ismpc_a_tick_kernel<false>, dim3(grid), dim3(T), sinv_bytes, s, h->c, (const ismpc_a_state*)h->prev, state_dev, push_dev, out_dev, batch, (double*)nullptr);
    HIP_TRY_A(hipGetLastError());
    return 0;
}

int ismpc_a_tick_batch_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const double* push_dev,
                              ismpc_a_out* out_dev, void* stream)
{
    return tick_launch(h, batch, state_dev, nullptr, push_dev, out_dev, stream);
}

int ismpc_a_set_precision(ismpc_a_handle* h, int fp32)
{
    if (!h) return fail_a(-1, "null handle");
    if (fp32 && (h->c.F < 3 || h->c.F > 6 || !h->use_wave)) return fail_a(-1, "the fp32 solve needs the structured kernel: 3 <= F <= 6");
    h->precision = fp32 ? 1 : 0; h->hist_valid = false;
    return 0;
}

int ismpc_a_last_deferred(ismpc_a_handle* h)
{
    if (!h) return fail_a(-1, "null handle");
    if (!h->used || h->precision != 1 || h->defer_off) return 0;
    ON_DEVICE_A(h);
    int n = 0;
    HIP_TRY_A(hipStreamSynchronize(h->last_stream));
    HIP_TRY_A(hipMemcpy(&n, h->work_counter + 2, sizeof(int), hipMemcpyDeviceToHost));
    return n;
}

int ismpc_a_set_warm_history(ismpc_a_handle* h, int enabled)
{
    if (!h) return fail_a(-1, "null handle");
    h->hist_ticks = enabled != 0; h->hist_valid = false;
    return 0;
}

int ismpc_a_tick_batch_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev,
                                   const double* push_dev, ismpc_a_out* out_dev, void* stream)
{
    if (batch > 0 && !inst_dev) return fail_a(-1, "null per-instance parameter array");
    return tick_launch(h, batch, state_dev, inst_dev, push_dev, out_dev, stream);
}

// ---- the tick's whole decision and predicted horizon
int ismpc_a_horizon_shape(const ismpc_a_handle* h, int* C, int* F)
{
    if (!h) return fail_a(-1, "ismpc_a_horizon_shape: null handle");
    if (!C || !F) return fail_a(-1, "ismpc_a_horizon_shape: null C or F");
    *C = h->c.C; *F = h->c.F;
    return 0;
}

int ismpc_a_tick_batch_horizon_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, const double* push_dev,
                                      ismpc_a_out* out_dev, double* dec_dev, double* pred_dev, void* stream)
{
    // every argument error before the handle is looked at, let alone the device (as ismpc_a_rollout_mc_device)
    if (batch < 0) return fail_a(-1, "ismpc_a_tick_batch_horizon_device: negative batch");
    if (!out_dev) return fail_a(-1, "ismpc_a_tick_batch_horizon_device: null out_dev (the prediction reads the tick's status from it)");
    if (!dec_dev) return fail_a(-1, "ismpc_a_tick_batch_horizon_device: null dec_dev");
    if (batch > 0 && !state_dev) return fail_a(-1, "ismpc_a_tick_batch_horizon_device: batch > 0 with a null state_dev");
    if (!h) return fail_a(-1, "ismpc_a_tick_batch_horizon_device: null handle");
    if (int rc = tick_launch(h, batch, state_dev, inst_dev, push_dev, out_dev, stream, -1, nullptr, dec_dev)) return rc;
    if (batch == 0 || !pred_dev) return 0;
    ON_DEVICE_A(h);
    const unsigned grid = (unsigned)((2ll * batch + HZ_PAIRS - 1) / HZ_PAIRS);
    hipLaunchKernelGGL(ismpc_a_predict_kernel, dim3(grid), dim3(HZ_PAIRS), 0, static_cast<hipStream_t>(stream), h->c, (const ismpc_a_state*)h->prev,
                       (const ismpc_a_state*)state_dev, inst_dev, (const ismpc_a::PiPre*)(inst_dev ? h->pre : nullptr), (const ismpc_a_out*)out_dev,
                       (const double*)dec_dev, pred_dev, batch);
    HIP_TRY_A(hipGetLastError());
    return 0;
}

int ismpc_a_feet_rows(const ismpc_a_handle* h) { return h ? h->feet.rows : -1; }

// The base foot plans on the device (nplans x (rows + 8) x 8: the walk script writes rows fc+1 .. fc+8, the last row is repeated) in place of
// the handle's previous ones, and the foot rules of every plan in dst[0 .. nplans).
static int feet_upload(ismpc_a_handle* h, const ismpc_a_gait* gaits, const double* plans_host, int rows, int nplans, FeetParams* dst)
{
    const int rp = rows + 8;
    std::vector<double> base((size_t)nplans * rp * 8);
    for (int k = 0; k < nplans; ++k)
        for (int r = 0; r < rp; ++r)
            std::memcpy(&base[((size_t)k * rp + r) * 8], plans_host + ((size_t)k * rows + std::min(r, rows - 1)) * 8, 64);
    if (h->feet_base) { (void)hipFree(h->feet_base); h->feet_base = nullptr; h->feet_base_plans = 0; }
    HIP_TRY_A(hipMalloc((void**)&h->feet_base, base.size() * sizeof(double)));
    HIP_TRY_A(hipMemcpy(h->feet_base, base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice));
    h->feet_base_plans = nplans;
    for (int k = 0; k < nplans; ++k) {
        FeetParams& f = dst[k];
        f.gait = gaits[k].gait; f.rows = rp; f.phi = gaits[k].phi; f.disp_i = gaits[k].disp_i; f.disp_o = gaits[k].disp_o; f.disp_forw = gaits[k].disp_forw;
    }
    return 0;
}
// ... and the rules where the feet kernels read them (ismpc_a_handle::feet_rules), after feet_upload's caller has settled h->feet
static int feet_rules_upload(ismpc_a_handle* h)
{
    if (!h->feet_rules) { HIP_TRY_A(hipMalloc((void**)&h->feet_rules, 5 * sizeof(FeetParams))); h->allocs.push_back(h->feet_rules); }
    FeetParams r[5] = {h->feet_set.p[0], h->feet_set.p[1], h->feet_set.p[2], h->feet_set.p[3], h->feet};
    HIP_TRY_A(hipMemcpy(h->feet_rules, r, sizeof(r), hipMemcpyHostToDevice));
    return 0;
}

int ismpc_a_feet_init_device(ismpc_a_handle* h, const ismpc_a_gait* g, const double* foot_plan_host, int rows, int batch,
                             double* feet_dev, void* stream)
{
    if (!h || !g || !foot_plan_host || rows < 2 || batch < 0 || (batch > 0 && !feet_dev)) return fail_a(-1, "bad argument");
    ON_DEVICE_A(h);
    if (int rc = feet_upload(h, g, foot_plan_host, rows, 1, &h->feet)) return rc;
    if (int rc = feet_rules_upload(h)) return rc;
    h->feet_from_table = false;
    const int rp = h->feet.rows;
    if (batch > 0) {
        hipLaunchKernelGGL(ismpc_a_feet_fill, dim3(std::min(1024, (int)(((size_t)batch * rp * 8 + 255) / 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
                           (const double*)h->feet_base, feet_dev, rp, batch);
        HIP_TRY_A(hipGetLastError());
    }
    return 0;
}

// Per-instance gait parameters (ismpc_a_inst): instance b follows the foot rules and starts from the foot plan of its base plan.
int ismpc_a_feet_init_inst_device(ismpc_a_handle* h, const ismpc_a_gait* gaits, const double* foot_plans_host, int rows, int nplans,
                                  int batch, const ismpc_a_inst* inst_dev, double* feet_dev, void* stream)
{
    if (!h || !gaits || !foot_plans_host || rows < 2 || nplans < 1 || nplans > 4 || batch < 0 || (batch > 0 && (!feet_dev || !inst_dev)))
        return fail_a(-1, "bad argument");
    if (h->table) return fail_a(-1, "ismpc_a_feet_init_inst_device: a plan-table handle starts its feet with ismpc_a_feet_init_plans_device (the table is the source)");
    if (nplans != h->c.nplans) return fail_a(-1, "feet: one gait record and one foot plan per base plan of the handle (ismpc_a_create + ismpc_a_add_plan)");
    ON_DEVICE_A(h);
    if (int rc = feet_upload(h, gaits, foot_plans_host, rows, nplans, h->feet_set.p)) return rc;
    h->feet_plans = nplans; h->feet = h->feet_set.p[0];
    if (int rc = feet_rules_upload(h)) return rc;
    const int rp = h->feet.rows;
    if (batch > 0) {
        hipLaunchKernelGGL(ismpc_a_feet_fill_inst, dim3(std::min(1024, (int)(((size_t)batch * rp * 8 + 255) / 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
                           h->feet_tab(true), inst_dev, feet_dev, rp, batch);
        HIP_TRY_A(hipGetLastError());
    }
    return 0;
}

// Plan-table handles: the blocks come from the table's foot plans, the rules are the table's (nothing is uploaded).
int ismpc_a_feet_init_plans_device(ismpc_a_handle* h, int rows, int batch, const ismpc_a_inst* inst_dev, double* feet_dev, void* stream)
{
    if (!h) return fail_a(-1, "ismpc_a_feet_init_plans_device: null handle");
    if (!h->table) return fail_a(-1, "ismpc_a_feet_init_plans_device: needs a handle of ismpc_a_create_plans");
    if (rows < 2 || rows > h->p.n_gait + 1) return fail_a(-1, "ismpc_a_feet_init_plans_device: rows must be in [2, n_gait + 1]");
    if (batch < 0 || (batch > 0 && !feet_dev)) return fail_a(-1, "ismpc_a_feet_init_plans_device: negative batch, or batch > 0 with a null feet_dev");
    ON_DEVICE_A(h);
    const int rp = rows + ISMPC_A_FEET_PAD;
    const ismpc_a_gait& g = h->gaits[0];
    h->feet.gait = g.gait; h->feet.rows = rp; h->feet.phi = g.phi; h->feet.disp_i = g.disp_i; h->feet.disp_o = g.disp_o; h->feet.disp_forw = g.disp_forw;
    h->feet_plans = h->c.nplans; h->feet_from_table = true;
    if (batch > 0) {
        hipLaunchKernelGGL(ismpc_a_feet_fill_inst, dim3(std::min(1024, (int)(((size_t)batch * rp * 8 + 255) / 256))), dim3(256), 0, static_cast<hipStream_t>(stream),
                           h->feet_tab(true), inst_dev, feet_dev, rp, batch);
        HIP_TRY_A(hipGetLastError());
    }
    return 0;
}

static int tick_feet(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, const double* push_dev,
                     ismpc_a_out* out_dev, double* feet_dev, void* stream, int history = -1, const McTick* mc = nullptr)
{
    if (!h || !out_dev || (batch > 0 && !feet_dev) || h->feet.rows == 0) return fail_a(-1, "feet: call ismpc_a_feet_init_device first and pass an output buffer");
    if (inst_dev && h->feet_plans == 0) return fail_a(-1, "feet: per-instance batches need ismpc_a_feet_init_inst_device");
    ON_DEVICE_A(h);                                                 // the feet launch below runs on the handle's device too
    int rc = tick_launch(h, batch, state_dev, inst_dev, push_dev, out_dev, stream, history, mc);
    if (rc || batch == 0) return rc;
    hipLaunchKernelGGL(ismpc_a_feet_kernel, dim3((batch + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       h->feet_tab(inst_dev != nullptr), inst_dev, (const ismpc_a_state*)h->prev, (const ismpc_a_out*)out_dev, feet_dev, h->feet.rows, batch);
    HIP_TRY_A(hipGetLastError());
    return 0;
}

int ismpc_a_tick_feet_batch_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const double* push_dev,
                                   ismpc_a_out* out_dev, double* feet_dev, void* stream)
{
    return tick_feet(h, batch, state_dev, nullptr, push_dev, out_dev, feet_dev, stream);
}

int ismpc_a_tick_feet_batch_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, const double* push_dev,
                                        ismpc_a_out* out_dev, double* feet_dev, void* stream)
{
    if (batch > 0 && !inst_dev) return fail_a(-1, "null per-instance parameter array");
    return tick_feet(h, batch, state_dev, inst_dev, push_dev, out_dev, feet_dev, stream);
}

// Closed loop of `ticks` ticks, the previous tick's working set as the first guess; with_feet: the swing-foot QPs after every tick.
static int rollout_a(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, int ticks, ismpc_a_out* traj_dev,
                     bool with_feet, double* feet_dev, void* stream)
{
    for (int t = 0; t < ticks; ++t) {
        ismpc_a_out* out = traj_dev ? traj_dev + (size_t)t * batch : nullptr;
        const int history = t == 0 ? 1 : 2;
        const int rc = with_feet ? tick_feet(h, batch, state_dev, inst_dev, nullptr, out, feet_dev, stream, history)
                                 : tick_launch(h, batch, state_dev, inst_dev, nullptr, out, stream, history);
        if (rc) return rc;
    }
    return 0;
}

int ismpc_a_rollout_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, int ticks, ismpc_a_out* out_traj_dev, void* stream)
{
    if (!h || batch < 0 || ticks < 0 || (batch > 0 && !state_dev)) return fail_a(-1, "bad argument");
    return rollout_a(h, batch, state_dev, nullptr, ticks, out_traj_dev, false, nullptr, stream);
}

int ismpc_a_rollout_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, int ticks,
                                ismpc_a_out* out_traj_dev, void* stream)
{
    if (!h || batch < 0 || ticks < 0) return fail_a(-1, "bad argument");
    if (ticks > 0 && batch > 0 && !inst_dev) return fail_a(-1, "null per-instance parameter array");
    return rollout_a(h, batch, state_dev, inst_dev, ticks, out_traj_dev, false, nullptr, stream);
}

// The disturbed closed loop: rollout_a's loop with ismpc_a_mc_prologue as every tick's prologue and one ismpc_a_mc_fold behind the last
// tick.  Tick t writes its output records into its trajectory row when it has one, into the handle's scratch records when only the
// summary wants them, and nowhere otherwise.
int ismpc_a_rollout_mc_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, int ticks,
                              const ismpc_a_push* pushes_dev, int n_push, int traj_stride, ismpc_a_out* traj_dev,
                              ismpc_a_rollout_summary* summary_dev, void* stream)
{
    // (what can be said about the numbers is said first: each message is reachable without a handle, i.e. without a device)
    if (batch < 0 || ticks < 0) return fail_a(-1, "ismpc_a_rollout_mc_device: negative batch or ticks");
    if (traj_stride < 1) return fail_a(-1, "ismpc_a_rollout_mc_device: traj_stride must be at least 1");
    if (n_push < 0) return fail_a(-1, "ismpc_a_rollout_mc_device: negative n_push");
    if (n_push > 0 && !pushes_dev) return fail_a(-1, "ismpc_a_rollout_mc_device: n_push > 0 with a null push table");
    if (batch > 0 && !state_dev) return fail_a(-1, "ismpc_a_rollout_mc_device: batch > 0 with a null state");
    if (!h) return fail_a(-1, "ismpc_a_rollout_mc_device: null handle");
    if (n_push == 0 && traj_stride == 1 && !summary_dev) return rollout_a(h, batch, state_dev, inst_dev, ticks, traj_dev, false, nullptr, stream);
    if (batch == 0) return 0;
    ON_DEVICE_A(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ismpc_host::StreamMark<ismpc_a_handle> mark_{h, s};
    if (batch > h->mc_cap) {                             // stream-ordered growth; ismpc_a_reserve sizes it beforehand
        ISMPC_GROW_ASYNC(fail_a, h, h->mc, h->mc_cap, batch, MC_BYTES_PER_INSTANCE * (size_t)batch, s);
    }
    double* const push = n_push > 0 ? reinterpret_cast<double*>(h->mc + h->mc_cap) : nullptr;
    ismpc_a_out* last = nullptr;                         // where the previous tick's records are
    for (int t = 0; t < ticks; ++t) {
        const bool recorded = traj_dev && (t + 1) % traj_stride == 0;
        ismpc_a_out* out = recorded ? traj_dev + (size_t)((t + 1) / traj_stride - 1) * batch : (summary_dev ? h->mc : nullptr);
        const McTick mc{pushes_dev, n_push, t, push, summary_dev ? last : nullptr, summary_dev};
        if (int rc = tick_launch(h, batch, state_dev, inst_dev, push, out, stream, t == 0 ? 1 : 2, &mc)) return rc;
        last = out;
    }
    if (summary_dev) {
        hipLaunchKernelGGL(ismpc_a_mc_fold, dim3((batch + 255) / 256), dim3(256), 0, s, (const ismpc_a_out*)last, summary_dev, batch, ticks - 1);
        HIP_TRY_A(hipGetLastError());
    }
    return 0;
}

// The disturbed closed loop with the swing-foot QPs: ismpc_a_rollout_mc_device's loop over tick_feet.  ismpc_a_feet_kernel reads the
// tick's f0 and status, so every tick has an output record: its trajectory row, else the handle's scratch records -- whether or not a
// summary wants them.  (ismpc_a_mc_prologue folds and clears those records in this order when two unrecorded ticks follow each other.)
int ismpc_a_rollout_mc_feet_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, int ticks,
                                   const ismpc_a_push* pushes_dev, int n_push, int traj_stride, ismpc_a_out* traj_dev,
                                   ismpc_a_rollout_summary* summary_dev, double* feet_dev, ismpc_a_feet_summary* feet_summary_dev, void* stream)
{
    if (batch < 0 || ticks < 0) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: negative batch or ticks");
    if (traj_stride < 1) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: traj_stride must be at least 1");
    if (n_push < 0) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: negative n_push");
    if (n_push > 0 && !pushes_dev) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: n_push > 0 with a null push table");
    if (batch > 0 && !state_dev) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: batch > 0 with a null state");
    if (batch > 0 && !feet_dev) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: batch > 0 with a null feet_dev");
    if (!h) return fail_a(-1, "ismpc_a_rollout_mc_feet_device: null handle");
    ON_DEVICE_A(h);
    if (h->feet.rows == 0) return fail_a(-1, "feet: call ismpc_a_feet_init_device first and pass an output buffer");
    if (inst_dev && h->feet_plans == 0) return fail_a(-1, "feet: per-instance batches need ismpc_a_feet_init_inst_device");
    if (batch == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ismpc_host::StreamMark<ismpc_a_handle> mark_{h, s};
    if (batch > h->mc_cap) {                             // stream-ordered growth; ismpc_a_reserve sizes it beforehand
        ISMPC_GROW_ASYNC(fail_a, h, h->mc, h->mc_cap, batch, MC_BYTES_PER_INSTANCE * (size_t)batch, s);
    }
    double* const push = n_push > 0 ? reinterpret_cast<double*>(h->mc + h->mc_cap) : nullptr;
    ismpc_a_out* last = nullptr;                         // where the previous tick's records are
    for (int t = 0; t < ticks; ++t) {
        const bool recorded = traj_dev && (t + 1) % traj_stride == 0;
        ismpc_a_out* out = recorded ? traj_dev + (size_t)((t + 1) / traj_stride - 1) * batch : h->mc;
        const McTick mc{pushes_dev, n_push, t, push, summary_dev ? last : nullptr, summary_dev};
        if (int rc = tick_feet(h, batch, state_dev, inst_dev, push, out, feet_dev, stream, t == 0 ? 1 : 2, &mc)) return rc;
        last = out;
    }
    if (summary_dev) {
        hipLaunchKernelGGL(ismpc_a_mc_fold, dim3((batch + 255) / 256), dim3(256), 0, s, (const ismpc_a_out*)last, summary_dev, batch, ticks - 1);
        HIP_TRY_A(hipGetLastError());
    }
    if (feet_summary_dev) {
        FeetTab ft = h->feet_tab(inst_dev != nullptr);
        if (ft.base == h->feet_base) ft.nplans = std::min(ft.nplans, h->feet_base_plans);     // the base plans the last ismpc_a_feet_init*_device left on the device
        hipLaunchKernelGGL(ismpc_a_feet_summary_kernel, dim3((batch + FEET_SUMMARY_WAVES - 1) / FEET_SUMMARY_WAVES), dim3(64 * FEET_SUMMARY_WAVES), 0, s,
                           (const double*)feet_dev, ft, inst_dev, h->feet.rows, batch, feet_summary_dev);
        HIP_TRY_A(hipGetLastError());
    }
    return 0;
}

int ismpc_a_rollout_feet_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, int ticks, ismpc_a_out* out_traj_dev,
                                double* feet_dev, void* stream)
{
    if (!h || !out_traj_dev || batch < 0 || ticks < 0) return fail_a(-1, "bad argument");
    return rollout_a(h, batch, state_dev, nullptr, ticks, out_traj_dev, true, feet_dev, stream);
}

int ismpc_a_rollout_feet_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev, int ticks,
                                     ismpc_a_out* out_traj_dev, double* feet_dev, void* stream)
{
    if (!h || !out_traj_dev || batch < 0 || ticks < 0 || (batch > 0 && !inst_dev)) return fail_a(-1, "bad argument");
    return rollout_a(h, batch, state_dev, inst_dev, ticks, out_traj_dev, true, feet_dev, stream);
}

// quad_as_bip_no_plots.m:482-509 / quad_walk_no_plots.m:562-613 (host)
int ismpc_a_foot_trajectories(const ismpc_a_gait* g, int step, const double* foot_plan, int rows, int sim_duration, double* dst)
{
    if (!g || !foot_plan || !dst || step < 1 || sim_duration < step) return fail_a(-1, "bad argument");
    const int nsteps = sim_duration / step, n = nsteps * step;
    if (nsteps + 1 > rows) return fail_a(-1, "foot_plan has too few rows for this duration");
    auto FPL = [&](int r, int c) { return foot_plan[(size_t)(r - 1) * 8 + (c - 1)]; };
    auto put = [&](int foot, int row, double x, double y, double z) { double* d = dst + ((size_t)foot * n + row) * 3; d[0] = x; d[1] = y; d[2] = z; };
    int row = 0, cont = 1;
    for (int i = 1; i <= nsteps; ++i) {
        if (g->gait == 0) {
            if (step <= 50) return fail_a(-1, "the trot writer assumes step_duration > 50 (30 + 50 rows per step)");
            for (int k = 1; k <= step - 50; ++k, ++row) {
                put(0, row, FPL(i,7), FPL(i,8), 0.0); put(3, row, FPL(i,3), FPL(i,4), 0.0); put(1, row, FPL(i,5), FPL(i,6), 0.0); put(2, row, FPL(i,1), FPL(i,2), 0.0);
            }
            for (int j = 1; j <= 50; ++j, ++row) {
                const double z = -0.000032 * j * j + 0.0016 * j;
                const int still1 = (i % 2 == 1) ? 7 : 1, still2 = (i % 2 == 1) ? 3 : 5, mv1 = (i % 2 == 1) ? 1 : 7, mv2 = (i % 2 == 1) ? 5 : 3;
                const int footOf[9] = {0, 2, 0, 3, 0, 1, 0, 0, 0};             // column -> file index (fl 0, fr 1, rl 2, rr 3)
                put(footOf[still1], row, FPL(i,still1), FPL(i,still1+1), 0.0); put(footOf[still2], row, FPL(i,still2), FPL(i,still2+1), 0.0);
                put(footOf[mv1], row, FPL(i,mv1) + (FPL(i+1,mv1) - FPL(i,mv1)) / 50 * j, FPL(i,mv1+1) + (FPL(i+1,mv1+1) - FPL(i,mv1+1)) / 50 * j, z);
                put(footOf[mv2], row, FPL(i,mv2) + (FPL(i+1,mv2) - FPL(i,mv2)) / 50 * j, FPL(i,mv2+1) + (FPL(i+1,mv2+1) - FPL(i,mv2+1)) / 50 * j, z);
            }
        } else {
            for (int k = 1; k <= step; ++k, ++row) {
                const double z = -0.000032 * k * k + 0.0016 * k;
                const int mv = (cont == 2) ? 7 : (cont == 4) ? 3 : (cont == 6) ? 5 : (cont == 8) ? 1 : 0;
                const int cols[4] = {7, 5, 1, 3};
                for (int ft = 0; ft < 4; ++ft) {
                    const int cc = cols[ft];
                    if (cc == mv) put(ft, row, FPL(i,cc) + (FPL(i+1,cc) - FPL(i,cc)) / step * k, FPL(i,cc+1) + (FPL(i+1,cc+1) - FPL(i,cc+1)) / step * k, z);
                    else put(ft, row, FPL(i,cc), FPL(i,cc+1), 0.0);
                }
            }
            cont = (cont == 8) ? 1 : cont + 1;
        }
    }
    return n;
}

// The same on the device for a whole batch (ismpc_a_foot_trajectories_kernel): every instance's refusal is its own nrows = -1.
int ismpc_a_foot_trajectories_device(ismpc_a_handle* h, int batch, const ismpc_a_inst* inst_dev, const double* feet_dev, int sim_duration,
                                     double* dst_dev, int32_t* nrows_dev, void* stream)
{
    if (batch < 0) return fail_a(-1, "ismpc_a_foot_trajectories_device: negative batch");
    if (sim_duration < 1) return fail_a(-1, "ismpc_a_foot_trajectories_device: sim_duration must be at least 1");
    if (batch > 0 && !feet_dev) return fail_a(-1, "ismpc_a_foot_trajectories_device: batch > 0 with a null feet_dev");
    if (batch > 0 && !dst_dev) return fail_a(-1, "ismpc_a_foot_trajectories_device: batch > 0 with a null dst_dev");
    if (!h) return fail_a(-1, "ismpc_a_foot_trajectories_device: null handle");
    ON_DEVICE_A(h);
    if (h->feet.rows == 0) return fail_a(-1, "feet: call ismpc_a_feet_init_device first and pass an output buffer");
    if (inst_dev && h->feet_plans == 0) return fail_a(-1, "feet: per-instance batches need ismpc_a_feet_init_inst_device");
    if (batch == 0) return 0;
    const int chunks = (sim_duration + FOOT_CHUNK_ROWS - 1) / FOOT_CHUNK_ROWS;
    if ((long long)batch * chunks > 0x7fffffffLL) return fail_a(-1, "ismpc_a_foot_trajectories_device: batch x sim_duration beyond one launch");
    const size_t lds = sizeof(double) * 8 * (size_t)std::min(h->feet.rows, FOOT_PLAN_ROWS);
    hipLaunchKernelGGL(ismpc_a_foot_trajectories_kernel, dim3(batch * chunks), dim3(FOOT_THREADS), lds, static_cast<hipStream_t>(stream),
                       h->feet_tab(inst_dev != nullptr), inst_dev, h->p.step, feet_dev, h->feet.rows, sim_duration, chunks, batch, dst_dev, nrows_dev);
    HIP_TRY_A(hipGetLastError());
    return 0;
}

// fprintf(file, '%d %d %d\n', row): MATLAB prints an integer-valued double with %d and anything else with %e
int ismpc_a_write_trajectory_txt(const char* path, const double* rows3, int n)
{
    if (!path || !rows3 || n < 0) return fail_a(-1, "bad argument");
    FILE* f = std::fopen(path, "w");
    if (!f) return fail_a(-1, std::string("cannot open ") + path);
    for (int r = 0; r < n; ++r) {
        for (int c = 0; c < 3; ++c) {
            const double v = rows3[(size_t)r * 3 + c];
            if (v == std::floor(v) && std::fabs(v) < 1e15) std::fprintf(f, "%lld", (long long)v); else std::fprintf(f, "%e", v);
            std::fputc(c == 2 ? '\n' : ' ', f);
        }
    }
    std::fclose(f);
    return 0;
}

}  // extern "C"
