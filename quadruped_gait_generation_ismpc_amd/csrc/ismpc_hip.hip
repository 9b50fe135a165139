// ISMPC (Formulation B) per-tick hot path on gfx950 (MI355X): kernels + the C ABI of include/ismpc.h.
//
// One launch = one MPCSolver::solve (reference AMR_code_DART/MPCSolver.cpp:204-430) for every instance of a batch.  The vertical
// QP (MPCSolver.cpp:220-278) has a constant Hessian, so its solve is folded into affine tables at ismpc_create (ismpc_tables.cpp;
// for parameter sweeps on the device, ismpc_sweep.hip); what a tick computes is the nonlinear rest: lambda_j (:296-309), the
// 2x2 suffix scan for phi_state / phi_input (:362-371) and the two horizontal QPs (:395-396) as exact knapsack solves.
// This file is ONE translation unit: the kernel families live in the headers below and are instantiated side by side here,
// because the same tick arithmetic is inlined into several of them and their results must agree bit for bit.
//
//   ismpc_wave_prims.hpp  DPP moves, wavefront prefix sum / sum / broadcast (shared with Formulation A)
//   ismpc_host.hpp        device guard, early return on a HIP error, stream-ordered scratch growth (shared by the three ABIs)
//   ismpc_b_common.hpp    DevConst, Walk / load_walk / gate_tick, sinhc_coshc, frcp, QState / QOut and their stores, stamps
//   ismpc_b_dense.hpp     ismpc_tick_dense: the per-tick MFMA solve, 16 instances per workgroup.  ISMPC_PATH=dense only (A/B)
//   ismpc_b_affine.hpp    one instance per wavefront from the affine tables: ismpc_tick_affine (ISMPC_PATH=wave, and every
//                         horizon 128 < N <= 256), the active-set solve of the inequality rows 0 <= S_bar_z u <= 1e4
//                         (:158-160; z_active_set), its launch ismpc_tick_affine_fallback and its callable forms fallback_call*
//   ismpc_b_group.hpp     the DEFAULT for N <= 128: several instances per wavefront, one group of LPI lanes each
//                         (ismpc_tick_quad, _inline, _one, ismpc_rollout_quad), and the sort of ismpc_sweep_bind
//   ismpc_tables.{hpp,cpp}  the host tables (long double) and lane_group_tables(), their re-striding for the lane-group kernels
//   this file             ismpc_handle; the dispatch: quad_shape() / quad_R() (shape), pick_layout() / quad_launch() (lanes, constants, grid),
//                         with_sw() (handle kind), launch(); the constructor in stages (read_knobs(), check_args(), upload_tables(),
//                         upload_plans() / pair_records() / sweep_records() / upload_records(), create_impl()); the extern "C" entry points
//
// Which kernel a step of the default path takes (launch() below; ISMPC_LPI / ISMPC_ONE_LAUNCH override):
//   lanes per instance   32 up to LPI32_BATCH = 2 048 instances, 16 up to LPI16_BATCH = 8 192, 8 beyond (closed loops keep 16)
//   samples per lane     the smallest instantiated R that covers N (the shape table at quad_R())
//   launch form          every wavefront resident at once (waves <= 8 per CU): ismpc_tick_quad_inline, one launch;
//                        larger batches: ismpc_tick_quad_one, one launch, unless a recent launch deferred instances -- then
//                        ismpc_tick_quad + ismpc_tick_affine_fallback; parameter sweeps: the SW = 1 instantiations of the latter two,
//                        multi-plan handles (ismpc_create_plans): their SW = 2 instantiations
//   closed loops         ismpc_rollout_quad, the whole loop in one launch (ISMPC_ROLLOUT=host: one launch per tick); its MC = true
//                        instantiations for ismpc_rollout_mc_device (pushes, trajectory stride, per-instance summaries)
//
// There is no CPU fallback in this file: every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include <new>
#include <memory>
#include <algorithm>
#include <type_traits>
#include "ismpc_tables.hpp"
#include "ismpc_sweep.hpp"
#include "ismpc_host.hpp"

// Floating-point contraction is OFF for this file: every fused multiply-add is written as fma().  The same tick arithmetic
// is inlined into several kernels (per-tick, one-launch, in-kernel rollout, resume) whose results must agree bit for bit,
// and implicit contraction is a per-context optimiser decision.  (The pragma covers the kernel headers included below it.)
#pragma clang fp contract(off)

#include "ismpc_b_common.hpp"
#include "ismpc_b_dense.hpp"
#include "ismpc_b_affine.hpp"
#include "ismpc_b_group.hpp"

namespace {

thread_local std::string g_err = "";
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr) ISMPC_HIP_TRY(fail, expr)
#define ON_DEVICE(h_) ISMPC_ON_DEVICE(fail, h_)
using ismpc_host::DeviceGuard;
using ismpc_host::grow_sync;

}  // namespace

struct ismpc_handle {
    ismpc::Tables t;
    DevConst c{};
    int device = 0;
    std::vector<void*> dev_allocs;
    // staging for the host-pointer entry point
    ismpc_tick_in* st_in = nullptr; ismpc_tick_out* st_out = nullptr; int st_cap = 0;
    ismpc_tick_in* pin_in = nullptr; ismpc_tick_out* pin_out = nullptr;   // host-mapped staging for small batches (PIN_BATCH records)
    bool pin_off = false;
    hipStream_t own_stream = nullptr;
    int host_mode = 3;                                          // ISMPC_HOST_MODE: bit 0 = kernel reads page-locked caller records in place, bit 1 = writes them in place
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing = false; bool timed_pending = false; double last_ms = 0.0;
    int* zseen_host = nullptr; // DevConst::zseen as the host sees it
    int one_launch = 2;       // 2: one launch per step (ismpc_tick_quad_inline up to the resident size; beyond it ismpc_tick_quad_one unless recent launches deferred instances); 1: only the former; 0: never; 3: always
    int force_waves = 0;      // dense path: 4, 8 or 16 wavefronts per workgroup (0 = 16)
    unsigned char* zmark = nullptr; int zmark_cap = 0; int launch_id = 0; bool z_fallback = true;
    int* zstop = nullptr; int zstop_cap = 0;     // in-kernel rollouts: tick at which an instance was handed to the resume launch (-1: never)
    ismpc_tick_out* mcrec = nullptr; int mcrec_cap = 0;   // ismpc_rollout_mc_device: one scratch record per instance (a tick that only the summary wants)
    bool dense_path = false;  // true: per-tick MFMA solve (ismpc_tick_dense); false: affine tables (ismpc_tick_affine)
    int cus = 0;              // compute units of the device (kernel variant selection); 0: never the one-launch variant
    bool quad_path = true;    // affine tables, several instances per wavefront (ismpc_tick_quad) where it applies; ISMPC_PATH=wave: one per wavefront
    int lpi = 16;             // lanes per instance of the quad kernels: 16 (four instances per wavefront), 8 (eight) or 32 (two); ISMPC_LPI
    bool lpi_auto = true;     // no ISMPC_LPI: 32 lanes per instance for batches of <= LPI32_BATCH instances (scripts/lpi_batch.py: 1 us of 9-10
                              // there, slower from 3 072 on), 16 otherwise; the tables exist in both layouts
    const double* vqT32 = nullptr; const double* tzgT32 = nullptr;
    const double* vqT8 = nullptr; const double* tzgT8 = nullptr;     // ... and 8 lanes per instance beyond LPI16_BATCH instances per launch
    const DevConst* sets8 = nullptr;                                  // sweep handles: the set records with the 8-lane tables (null: 16 lanes at every batch size)
    const DevConst* sets32 = nullptr;                                 // multi-plan handles that choose the layout per launch: the pair records with the 32-lane tables
    int nplans = 0;               // ismpc_create_plans: P footstep plans, c.sets = one record per (set, plan) pair; 0 for every other handle
    std::vector<double> pl_midx, pl_midy;                             // ... and the host copy of every plan's midpoint columns (P x nmid each)
    int plans() const { return nplans ? nplans : 1; }
    bool kernel_rollout = true;   // closed loops run inside one launch (ismpc_rollout_quad); ISMPC_ROLLOUT=host: one launch per tick
    const DevConst* c_dev = nullptr;   // the constants in device memory (the one-launch kernel's fallback call reads them there)
    bool sweep = false;           // ismpc_create_sweep: K parameter sets, tables built on the device (csrc/ismpc_sweep.hip)
    ismpc::SweepSlabs sw; std::vector<ismpc_params> sets; std::vector<double> ftsp;   // (the plan as given: ismpc_sweep_verify_tables rebuilds a set on the host)
    int* order = nullptr; int order_cap = 0, order_batch = 0;   // ismpc_sweep_bind: instances of the bound batch sorted by parameter set (+ nsets + 1 bucket cursors)
    int last_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};             // ismpc_last_launch_info: what the most recent step or rollout enqueued (plain host stores)
    hipStream_t last_stream = nullptr; bool used = false;   // stream of the previous launch: zmark / zstop outlive a call and are re-allocated
                                                            // only after that stream has drained (grow_sync)
};

namespace {

template <typename T>
int upload(ismpc_handle* h, const std::vector<T>& v, const T** dst)
{
    void* p = nullptr;
    size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    HIP_TRY(hipMalloc(&p, bytes));
    h->dev_allocs.push_back(p);
    if (!v.empty()) HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return ISMPC_OK;
}

// Shape of the lane-group kernels for horizon N: samples per lane R (the smallest instantiated value that covers N) for
// LPI = 16 / 8 lanes per instance; RW = samples per lane of the one-instance-per-wavefront fallback body.
constexpr int LPI32_BATCH = 2048;
// ... 8 lanes per instance (eight instances per wavefront, 13 samples per lane at N = 100, two wavefronts per SIMD) beyond this many:
// a launch that does not fit the chip at once is bound by the instructions it issues, and a group reduction or scan step serves twice
// the instances (round 3, one box: 65 536 instances 1.30-1.35 -> 1.41-1.44e9 ticks/s, 32 768 1.18 -> 1.24e9, 16 384 0.94 -> 1.03e9;
// 8 192 level, 1 024 slower)
constexpr int LPI16_BATCH = 8192;
// Zero double2 entries behind the last plan of every midxy table.  The lane-group kernels stage the window [idx, idx + LPI R) of an instance
// without a clamp (tick_group_core); the gate admits idx <= nmid - 2 N, so the largest entry read is nmid - 2 N + LPI R - 1 of the instance's
// plan -- past the table's end by at most LPI R - 2 N <= 126 entries (N >= 1; LPI R <= 128 in every shape of quad_shape()).
constexpr size_t MIDXY_SLACK = 128;
struct LaneLayout { int lpi; const double* vqT; const double* tzgT; };
// THE shape table: calls f(R, LPI, RW) with the compile-time shape (std::integral_constant arguments) of horizon N at lpi lanes
// per instance, and returns what f returns.  Every launch of a lane-group kernel and quad_R() go through it.
template <int R, int LPI, int RW, class F> auto with_shape(F&& f)
{
    static_assert((size_t)R * LPI <= MIDXY_SLACK, "the unclamped midpoint window of this shape needs more slack behind the midxy tables");
    return f(std::integral_constant<int, R>{}, std::integral_constant<int, LPI>{}, std::integral_constant<int, RW>{});
}
template <class F> auto quad_shape(int N, int lpi, F&& f)
{
    const int need = (N + lpi - 1) / lpi;
    if (lpi == 32) return N <= 64 ? with_shape<4, 32, 1>(f) : with_shape<4, 32, 2>(f);
    if (lpi == 16) return need <= 4 ? with_shape<4, 16, 1>(f) : (need <= 7 ? with_shape<7, 16, 2>(f) : with_shape<8, 16, 2>(f));
    return need <= 8 ? with_shape<8, 8, 1>(f) : (need <= 13 ? with_shape<13, 8, 2>(f) : with_shape<16, 8, 2>(f));
}
int quad_R(int N, int lpi) { return quad_shape(N, lpi, [](auto R, auto, auto) { return (int)R; }); }
// ... and of the one-instance-per-wavefront kernels (R = ceil(N / 64) samples per lane): false beyond the instantiated N <= 256
template <class F> bool wave_shape(int R, F&& f)
{
    switch (R) {
        case 1: f(std::integral_constant<int, 1>{}); return true;
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 3: f(std::integral_constant<int, 3>{}); return true;
        case 4: f(std::integral_constant<int, 4>{}); return true;
    }
    return false;
}

// Lanes per instance of a launch of `batch` instances (the handle's own layout unless it chooses per launch: no ISMPC_LPI, no sweep).
// per_tick = false: the closed loop (ismpc_rollout_device, in the kernel or one launch per tick) keeps the 16-lane shape beyond LPI32_BATCH --
// with the state in registers across ticks it is the faster one there too (65 536 instances: 1.72 against 1.61e9 ticks/s).  Layouts differ in
// summation order, i.e. in the last bits: a tick of ismpc_solve_batch* and a tick of a rollout agree to rounding, not to the byte, beyond
// LPI16_BATCH instances per launch.
LaneLayout pick_layout(const ismpc_handle* h, int batch, bool per_tick)
{
    if (h->lpi_auto && h->vqT32 && batch <= LPI32_BATCH) return {32, h->vqT32, h->tzgT32};
    if ((h->lpi_auto || (h->sweep && h->sets8)) && h->vqT8 && per_tick && batch > LPI16_BATCH) return {8, h->vqT8, h->tzgT8};
    return {h->lpi, h->c.vqT, h->c.tzgT};
}
// What kind of handle it is, in the one place that says so.  The kernels take it as their SW template argument -- 2: a multi-plan handle
// (each instance's (set, plan) pair through c.sets), 1: a parameter sweep (each instance's set through c.sets), 0: neither -- and
// ismpc_last_launch_info as its form bits (bit 0 = sweep, bit 1 = multi-plan instantiation).  with_sw() calls f(SW) with the compile-time value and returns what f returns.
int form_bits(const ismpc_handle* h) { return (h->sweep ? 1 : 0) | (h->nplans ? 2 : 0); }
template <class F> auto with_sw(const ismpc_handle* h, F&& f)
{
    if (h->nplans) return f(std::integral_constant<int, 2>{});
    if (h->sweep) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, 0>{});
}
// Which (lanes per instance, SW) pairs the lane-group kernels are instantiated for: SW = 0 and SW = 2 at every lane count; SW = 1 at 16 and
// 8 lanes for the tick kernels and at 16 lanes only for the rollout (a sweep handle takes no other: create_impl() gives it 16, pick_layout() 8)
constexpr bool has_tick_quad(int lpi, int sw) { return sw != 1 || lpi != 32; }
constexpr bool has_rollout_quad(int lpi, int sw) { return sw != 1 || lpi == 16; }

// What a launch of a lane-group kernel needs, for launch() and ismpc_rollout_device(): the lanes per instance of pick_layout(), the constants
// with that layout's affine tables and set records, the order of ismpc_sweep_bind where it applies, and the grid.
// (width(): grid and block at `wpg` wavefronts per workgroup -- ISMPC_QUAD_WAVES for the rollout, tick_wpg() of the shape for the per-tick kernels)
struct QuadLaunch {
    int lpi, waves; dim3 grid, block; DevConst c;
    void width(int wpg) { grid = dim3((waves + wpg - 1) / wpg); block = dim3(64 * wpg); }
};
// (sweep and multi-plan handles: the records that go with the lane layout; a plain handle has none)
const DevConst* sets_for(const ismpc_handle* h, int lpi)
{
    return (lpi == 8 && h->sets8) ? h->sets8 : ((lpi == 32 && h->sets32) ? h->sets32 : h->c.sets);
}
QuadLaunch quad_launch(const ismpc_handle* h, int batch, bool per_tick)
{
    const LaneLayout lay = pick_layout(h, batch, per_tick);
    QuadLaunch q{lay.lpi, (batch * lay.lpi + 63) / 64, dim3(), dim3(), h->c};
    q.width(ISMPC_QUAD_WAVES);
    q.c.vqT = lay.vqT; q.c.tzgT = lay.tzgT;
    q.c.sets = sets_for(h, lay.lpi);
    // (ismpc_sweep_bind; per-tick launches of the bound batch only, and never a plain handle: ismpc_sweep_bind refuses it)
    q.c.order = (h->order && h->order_batch == batch && per_tick && form_bits(h) != 0) ? h->order : nullptr;
    return q;
}
// Page-locked AND device-mapped over its whole length: both ends of [p, p + bytes) are host allocations known to the runtime and the
// device addresses of the two ends are `bytes - 1` apart (one mapping, or adjacent ones that continue each other).  A registration that
// covers only the head of the buffer, or an interior pointer near the end of a pinned block, fails this and takes the staged path
// instead of letting the kernel touch unmapped host memory over PCIe.
bool host_is_pinned(const void* p, size_t bytes)
{
    if (!p || bytes == 0) return false;
    hipPointerAttribute_t a, b;
    const char* last = static_cast<const char*>(p) + (bytes - 1);
    if (hipPointerGetAttributes(&a, p) != hipSuccess || hipPointerGetAttributes(&b, last) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeHost || b.type != hipMemoryTypeHost) return false;
    return a.devicePointer && b.devicePointer && static_cast<const char*>(b.devicePointer) - static_cast<const char*>(a.devicePointer) == (ptrdiff_t)(bytes - 1);
}
using StreamMark = ismpc_host::StreamMark<ismpc_handle>;

int launch(ismpc_handle* h, int batch, const ismpc_tick_in* in, ismpc_tick_in* state, ismpc_tick_out* out,
           double* u_traj, int rollout_frame, hipStream_t s)
{
    if (batch <= 0) return ISMPC_OK;
    StreamMark mark_{h, s};
    const int R = (h->c.N + 63) / 64;
    // the argument list every tick kernel starts with; `more`: zmark and the launch id, then the constants in device memory (one-launch forms)
    auto tick = [&](auto kernel, dim3 g, dim3 b, size_t lds, const DevConst& c, auto... more) {
        hipLaunchKernelGGL(kernel, g, b, lds, s, c, in, state, out, u_traj, batch, rollout_frame, more...);
    };
    // what this step enqueues, for ismpc_last_launch_info: written where the kernel is launched, from the same shape values
    auto note = [&](int family, int lanes, int r, int rw, int kernels, bool ordered) {
        const int v[8] = {family, lanes, r, rw, form_bits(h), kernels, batch, ordered ? 1 : 0};
        std::memcpy(h->last_launch, v, sizeof(v));
    };
    if (!h->dense_path) {
        // fast path: wavefront per instance, 4 per workgroup; then the (normally empty) inequality fallback
        const dim3 grid((batch + 3) / 4), block(256);
        if (h->z_fallback && batch > h->zmark_cap) {
            // stream-ordered growth (no device-wide synchronisation inside an asynchronous entry point); callers that
            // capture graphs size it beforehand with ismpc_reserve
            ISMPC_GROW_ASYNC(fail, h, h->zmark, h->zmark_cap, batch, zscratch_bytes(batch), s);
        }
        unsigned char* zm = h->z_fallback ? h->zmark : nullptr;
        const int lid = ++h->launch_id;
        const dim3 fgrid(std::min((batch + 3) / 4, 256));      // the fallback walks the list of deferred instances: one wavefront each
        // Batches beyond the resident size: ONE launch (ismpc_tick_quad_one: a wavefront that defers an instance runs the fallback for it
        // itself) while nothing is being deferred -- the usual case, and the second launch would be idle; TWO launches (the deferred
        // list, one wavefront per deferred instance at the fallback's own register budget) when one of the last few launches did defer:
        // measured on the sweep batch (0.4 % deferred) 70.5 against 75.8 us per step.  The kernels leave the id of a deferring launch in
        // a word of host memory; reading it here costs nothing.  The host enqueues far ahead of the device (a closed loop of per-tick
        // launches is hundreds of launches deep), so the word is stale by that much: `recent` is the last 4 096 launches.  Both forms
        // give the same bytes, so a late switch costs microseconds, never correctness.
        const bool recent_deferrals = h->zseen_host && *(volatile int*)h->zseen_host != 0 && lid - *(volatile int*)h->zseen_host <= 4096;
        const bool one_big = zm && (h->one_launch == 3 || (h->one_launch == 2 && !recent_deferrals));
        auto fallback = [&](auto RR, auto SW) { tick(ismpc_tick_affine_fallback<RR, SW>, fgrid, block, 0, h->c, zm, lid); };      // (the handle's own constants, not the lane-group launch's: one instance per wavefront)
        // default for N <= 128: several instances per wavefront (ismpc_tick_quad); ISMPC_PATH=wave keeps one per wavefront
        if (h->quad_path && h->c.N <= 128) {
            QuadLaunch q = quad_launch(h, batch, rollout_frame < 0);      // (a closed loop driven from the host keeps the in-kernel loop's layout: same bytes)
            // every wavefront resident at once (<= 2 per SIMD) and a fallback to run: one launch that handles deferred instances itself (plain handles: the
            // resident kernel has no SW instantiations)
            const bool resident = form_bits(h) == 0 && zm && h->one_launch >= 1 && h->cus > 0 && q.waves <= 8 * h->cus;
            // The launch forms, in this order: plain handles take ismpc_tick_quad_inline while the batch is resident; every handle then one
            // launch (ismpc_tick_quad_one, at the tick's own three wavefronts per SIMD) or tick + fallback launch, by one_big above.  A sweep
            // reads each instance's set through c.sets; a multi-plan handle its (set, plan) pair, in the records of this launch's layout -- its
            // lanes per instance are a plain handle's with one parameter set (whose records are then byte-identical to a plain handle's on
            // that plan) and a sweep's with several.
            const int rc = with_sw(h, [&](auto SW) {
                constexpr int sw = decltype(SW)::value;
                return quad_shape(h->c.N, q.lpi, [&](auto RR, auto LL, auto RW_) {
                    if constexpr (has_tick_quad(LL, sw)) {
                        q.width(resident ? tick_wpg<RR, LL, true>() : tick_wpg<RR, LL, false, sw>());      // (the workgroup of the kernel launched below)
                        if (resident) {
                            tick(ismpc_tick_quad_inline<RR, LL, RW_>, q.grid, q.block, 0, q.c, zm, lid, h->c_dev);
                            note(ISMPC_KERNEL_QUAD_INLINE, LL, RR, RW_, 1, q.c.order != nullptr);
                        } else if (one_big) {
                            tick(ismpc_tick_quad_one<RR, LL, RW_, sw>, q.grid, q.block, 0, q.c, zm, lid, h->c_dev);
                            note(ISMPC_KERNEL_QUAD_ONE, LL, RR, RW_, 1, q.c.order != nullptr);
                        } else {
                            tick(ismpc_tick_quad<RR, LL, sw>, q.grid, q.block, 0, q.c, zm, lid);
                            if (zm) fallback(RW_, SW);              // (RW = ceil(N / 64), the fallback's own samples per lane)
                            note(ISMPC_KERNEL_QUAD, LL, RR, RW_, zm ? 2 : 1, q.c.order != nullptr);
                        }
                        return ISMPC_OK;
                    } else
                        return fail(ISMPC_E_UNSUPPORTED, "parameter sweep: 16 or 8 lanes per instance");
                });
            });
            if (rc != ISMPC_OK) return rc;
            HIP_TRY(hipGetLastError());
            return ISMPC_OK;
        }
        const dim3 agrid((batch + ISMPC_AFF_WAVES - 1) / ISMPC_AFF_WAVES), ablock(64 * ISMPC_AFF_WAVES);
        auto affine = [&](auto RR) {
            with_sw(h, [&](auto SW) {
                tick(ismpc_tick_affine<decltype(RR)::value, decltype(SW)::value>, agrid, ablock, 0, h->c, zm, lid);
                if (zm) fallback(RR, SW);
            });
            note(ISMPC_KERNEL_AFFINE, 64, RR, RR, zm ? 2 : 1, false);
        };
        if (!wave_shape(R, affine)) return fail(ISMPC_E_UNSUPPORTED, "horizon N > 256");
        HIP_TRY(hipGetLastError());
        return ISMPC_OK;
    }
    // dense path (kept for A/B and as the per-tick MFMA formulation): 16 instances per workgroup
    const dim3 grid((batch + TI - 1) / TI);
    const size_t lds = (size_t)TI * h->c.NPs * sizeof(double);
    const int waves = h->force_waves ? h->force_waves : 16;
    auto dense = [&](auto RR) {
        if (waves == 16)     tick(ismpc_tick_dense<RR, 16>, grid, dim3(64 * 16), lds, h->c);
        else if (waves == 8) tick(ismpc_tick_dense<RR, 8>, grid, dim3(64 * 8), lds, h->c);
        else                 tick(ismpc_tick_dense<RR, 4>, grid, dim3(64 * 4), lds, h->c);
        note(ISMPC_KERNEL_DENSE, 64, RR, 0, 1, false);
    };
    if (!wave_shape(R, dense)) return fail(ISMPC_E_UNSUPPORTED, "horizon N > 256");
    HIP_TRY(hipGetLastError());
    return ISMPC_OK;
}

// The environment as ismpc_create* finds it: every knob that is read at creation, read once.  (ISMPC_PINNED and ISMPC_HOST_ALLOC_FLAGS
// are read by the calls they steer.)
struct Knobs {
    int force_waves = 0;            // ISMPC_WAVES: wavefronts per workgroup of the dense path, 4, 8 or 16 (tuning knob)
    bool dense = false, wave = false;   // ISMPC_PATH=dense | wave
    bool z_fallback = true;         // ISMPC_Z_FALLBACK=0: flag only, no second launch
    int lpi = 0;                    // ISMPC_LPI: 8, 16 or 32 lanes per instance (0: not given, the layout follows the batch size)
    bool kernel_rollout = true;     // ISMPC_ROLLOUT=host: one launch per tick
    int one_launch = 2;             // ISMPC_ONE_LAUNCH, A/B: 0 = always two launches, 1 = one launch only for batches resident at once, 3 = always one
    int host_mode = 3;              // ISMPC_HOST_MODE
    int zldsq = Z_LDS_Q;            // ISMPC_Z_LDS_Q
};
Knobs read_knobs()
{
    Knobs k;
    if (const char* fw = std::getenv("ISMPC_WAVES")) { const int v = std::atoi(fw); if (v == 4 || v == 8 || v == 16) k.force_waves = v; }
    if (const char* pth = std::getenv("ISMPC_PATH")) { k.dense = std::strcmp(pth, "dense") == 0; k.wave = std::strcmp(pth, "wave") == 0; }
    if (const char* zf = std::getenv("ISMPC_Z_FALLBACK")) k.z_fallback = std::atoi(zf) != 0;
    if (const char* lp = std::getenv("ISMPC_LPI")) { const int v = std::atoi(lp); if (v == 8 || v == 16 || v == 32) k.lpi = v; }
    if (const char* ro = std::getenv("ISMPC_ROLLOUT")) k.kernel_rollout = std::strcmp(ro, "host") != 0;
    if (const char* fu = std::getenv("ISMPC_ONE_LAUNCH")) k.one_launch = std::max(0, std::min(3, std::atoi(fu)));
    if (const char* hm = std::getenv("ISMPC_HOST_MODE")) k.host_mode = std::atoi(hm) & 3;
    if (const char* e = std::getenv("ISMPC_Z_LDS_Q")) k.zldsq = std::min(Z_LDS_Q, std::max(1, std::atoi(e)));
    return k;
}

// Everything that can be said about the arguments of ismpc_create, ismpc_create_plans (P > 0) and ismpc_create_sweep, said before the device is touched
int check_args(const ismpc_params* params, int K, bool sweep, const double* ftsp, int rows, int P, const Knobs& knobs)
{
    // every handle: the inequality fallback keeps the e-th pinned sample of an equality pattern in lane e of its wavefront (z_fetch / z_project,
    // ismpc_b_affine.hpp), and a pattern pins up to min(F, N) samples
    if (params[0].F > ISMPC_F_MAX) return fail(ISMPC_E_UNSUPPORTED, "F > 64 double-support samples: the vertical fallback holds one pinned sample per lane of a wavefront");
    if (P) {
        if (P < 1 || P > 32767) return fail(ISMPC_E_INVALID, "a multi-plan handle holds 1 .. 32767 footstep plans");
        if (K < 1 || K > 65535) return fail(ISMPC_E_INVALID, "a multi-plan handle holds 1 .. 65535 parameter sets");
        if (rows < 2) return fail(ISMPC_E_INVALID, "footstep plan needs at least 2 rows");
        if ((long long)K * P > (1ll << 24)) return fail(ISMPC_E_ALLOC, "more (set, plan) pairs than one handle holds (2^24: each pair has its own anticipative tails)");
        for (int p = 1; p < P; ++p)
            for (int i = 0; i < rows; ++i)
                if (std::memcmp(&ftsp[((size_t)p * rows + i) * 4 + 2], &ftsp[(size_t)i * 4 + 2], sizeof(double)) != 0)
                    return fail(ISMPC_E_UNSUPPORTED, "multi-plan handle: plan " + std::to_string(p) + " differs from plan 0 in the z column (row " + std::to_string(i) +
                                                     "); the plans of one handle share one height profile");
        if (knobs.dense) return fail(ISMPC_E_UNSUPPORTED, "multi-plan handle: ISMPC_PATH=dense reads one plan");
    }
    if (sweep) {
        // the sets of a sweep share what fixes the shape of the problem; everything else may differ from set to set
        if (K < 1 || K > 65535) return fail(ISMPC_E_INVALID, "a sweep holds 1 .. 65535 parameter sets");
        for (int k = 0; k < K; ++k) {
            const ismpc_params& a = params[0]; const ismpc_params& b = params[k];
            if (a.N != b.N || a.S != b.S || a.F != b.F || a.M != b.M || a.mpc_dt != b.mpc_dt || a.control_dt != b.control_dt || a.g != b.g || a.lambda_gate != b.lambda_gate)
                return fail(ISMPC_E_INVALID, "the parameter sets of a sweep share N, S, F, M, mpc_dt, control_dt, g and lambda_gate");
            if (!(b.mass > 0) || !(b.h_des > 0) || !(b.q_u > 0) || b.q_p < 0 || b.q_v < 0) return fail(ISMPC_E_INVALID, "sweep: mass, h_des, q_u must be positive, q_p and q_v non-negative");
        }
    }
    return ISMPC_OK;
}

// upload() of each (vector, destination) pair in turn, up to the first that fails
template <class V, class D, class... Rest> int upload_all(ismpc_handle* h, const V& v, D dst, const Rest&... rest)
{
    const int rc = upload(h, v, dst);
    if constexpr (sizeof...(rest) == 0) return rc;
    else return rc != ISMPC_OK ? rc : upload_all(h, rest...);
}
// DevConst records (pair records, set records, the handle's own constants) to device memory the handle owns
int upload_records(ismpc_handle* h, const std::vector<DevConst>& recs, const DevConst** dst, const char* what)
{
    void* p = nullptr;
    const size_t bytes = sizeof(DevConst) * recs.size();
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ISMPC_E_ALLOC, std::string(what) + ": records allocation failed"); }
    h->dev_allocs.push_back(p);
    if (hipMemcpy(p, recs.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(ISMPC_E_NO_DEVICE, std::string(what) + ": records upload failed");
    *dst = static_cast<const DevConst*>(p);
    return ISMPC_OK;
}

// The scalars of the constants, from the host tables
void fill_constants(const ismpc::Tables& t, int zldsq, DevConst& c)
{
    c.N = t.p.N; c.NP = t.NP; c.NPs = t.NP + 2; c.S = t.p.S; c.F = t.p.F; c.nmid = t.nmid; c.npat = t.npat;
    c.Fmax = t.Fmax; c.rows = t.rows; c.tick_divisor = t.tick_divisor;
    c.dt = t.p.mpc_dt; c.cdt = t.p.control_dt; c.mass = t.p.mass; c.g = t.p.g; c.h_des = t.p.h_des;
    c.half_run = t.p.foot_width / 2; c.half_first = t.p.first_step_halfwidth;
    c.q_p = t.p.q_p; c.q_u = t.p.q_u; c.q_v = t.p.q_v; c.z_lo = t.p.z_ineq_lo; c.z_hi = t.p.z_ineq_hi;
    c.gate = t.p.lambda_gate; c.eta = t.eta;
    c.inv_mass = 1.0 / t.p.mass; c.dt_over_mass = t.p.mpc_dt / t.p.mass; c.inv_eta = 1.0 / t.eta;
    c.sim_div = t.p.mpc_dt / t.p.control_dt; c.cdt_over_dt = t.p.control_dt / t.p.mpc_dt;
    c.flat = t.flat ? 1 : 0;
    // active-set fallback pool: 256 slots of (cap x cap + 4 cap + NT) doubles + cap ints, cap = N rows (every row may be active)
    c.zslots = 256; c.zcap = t.p.N; c.zldsq = zldsq;
    c.zstride = (size_t)c.zcap * c.zcap + 4 * (size_t)c.zcap + ismpc::Tables::NT + ((size_t)c.zcap + 1) / 2 + 8;
}

// The host tables, the fallback's scratch and the affine tables in the kernels' layouts, to the device.  all_layouts: the handle chooses
// its lanes per instance per launch (or is a sweep), so the 32-lane and the 8-lane copy go beside the handle's own
int upload_tables(ismpc_handle* h, bool all_layouts)
{
    const ismpc::Tables& t = h->t;
    DevConst& c = h->c;
    const std::vector<int> zf(4, 0), busy(c.zslots, 0); const int *zp = nullptr, *bp = nullptr;
    int rc = upload_all(h, t.Hinv, &c.Hinv, t.W, &c.W, t.midx, &c.midx, t.midy, &c.midy, t.midz, &c.midz, t.tailx, &c.tailx, t.taily, &c.taily,
                        t.ftsp_t, &c.ftsp_t, t.e_lo, &c.e_lo, t.ne, &c.ne, t.vtab, &c.vtab, t.tz, &c.tz, t.tg, &c.tg, t.dU, &c.dU, t.SdU, &c.SdU,
                        t.Wt, &c.Wt, t.SW, &c.SW, t.HSt, &c.HSt, t.SHSt, &c.SHSt, zf, &zp);
    if (rc != ISMPC_OK) return rc;
    c.zflag = const_cast<int*>(zp);
    {
        // one word of page-locked host memory the kernels write the launch id to when they defer an instance (see launch())
        void* hp = nullptr; void* dp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
            h->zseen_host = static_cast<int*>(hp); *h->zseen_host = 0; c.zseen = static_cast<int*>(dp);
        } else { if (hp) (void)hipHostFree(hp); (void)hipGetLastError(); c.zseen = nullptr; }
    }
    rc = upload(h, busy, &bp);                 // the active-set fallback pool and its slot flags
    if (rc != ISMPC_OK) return rc;
    c.zbusy = const_cast<int*>(bp);
    void* pool = nullptr;
    if (hipMalloc(&pool, c.zstride * c.zslots * sizeof(double)) != hipSuccess) return fail(ISMPC_E_ALLOC, "fallback pool allocation failed");
    h->dev_allocs.push_back(pool); c.zpool = static_cast<double*>(pool);
    constexpr int NTq = ismpc::Tables::NT;
    const size_t npp = t.vtab.size() / (6 * (size_t)NTq);
    std::vector<double> vq(t.vtab.size()), tzg(2 * (size_t)NTq), mxy(2 * (t.midx.size() + MIDXY_SLACK), 0.0);
    for (size_t pp = 0; pp < npp; ++pp)
        for (int k = 0; k < 6; ++k)
            for (int n = 0; n < NTq; ++n) vq[(pp * NTq + n) * 6 + k] = t.vtab[(pp * 6 + k) * NTq + n];
    for (int n = 0; n < NTq; ++n) { tzg[2 * n] = t.tz[n]; tzg[2 * n + 1] = t.tg[n]; }
    for (size_t n = 0; n < t.midx.size(); ++n) { mxy[2 * n] = t.midx[n]; mxy[2 * n + 1] = t.midy[n]; }
    rc = upload_all(h, vq, &c.vq, tzg, &c.tzg, mxy, &c.midxy);
    // lane-contiguous copies for the lane-group kernels' shapes (sample li*R + r of pattern p): the handle's layout and,
    // when the layout is chosen per launch, the 32-lane and the 8-lane one beside it
    const int layouts = t.p.N > 128 ? 0 : (all_layouts ? 3 : 1);
    for (int pass = 0; pass < layouts && rc == ISMPC_OK; ++pass) {
        const int lpi = pass == 0 ? h->lpi : (pass == 1 ? 32 : 8);
        std::vector<double> vqT, tzgT;
        ismpc::lane_group_tables(t, lpi, quad_R(t.p.N, lpi), vqT, tzgT);
        rc = upload_all(h, vqT, pass == 0 ? &c.vqT : (pass == 1 ? &h->vqT32 : &h->vqT8), tzgT, pass == 0 ? &c.tzgT : (pass == 1 ? &h->tzgT32 : &h->tzgT8));
    }
    return rc;
}

// Multi-plan handles, part 1: every plan's tables side by side on the device -- midx, midy, midxy (the lane-group kernels' window), the
// step timings and, with ONE parameter set, the host-built tails (with several the tails are built on the device per pair: sweep_build)
struct PlanSlabs { const double *midx = nullptr, *midy = nullptr, *midxy = nullptr, *t = nullptr, *tailx = nullptr, *taily = nullptr; };
int upload_plans(ismpc_handle* h, const ismpc_params& p0, const double* ftsp, PlanSlabs& pl)
{
    const int P = h->nplans, rows = h->t.rows; const bool sweep = h->sweep;
    const size_t nm = (size_t)h->t.nmid;
    std::vector<double> mxy(2 * (nm * P + MIDXY_SLACK), 0.0), tt((size_t)rows * P), tx(sweep ? 0 : nm * P), ty(sweep ? 0 : nm * P);
    h->pl_midx.resize(nm * P); h->pl_midy.resize(nm * P);
    for (int p = 0; p < P; ++p) {
        ismpc::PlanTables pt;
        ismpc::build_plan_tables(p0, ftsp + (size_t)p * rows * 4, rows, pt);
        std::copy(pt.midx.begin(), pt.midx.end(), h->pl_midx.begin() + p * nm); std::copy(pt.midy.begin(), pt.midy.end(), h->pl_midy.begin() + p * nm);
        for (size_t n = 0; n < nm; ++n) { mxy[2 * (p * nm + n)] = pt.midx[n]; mxy[2 * (p * nm + n) + 1] = pt.midy[n]; }
        std::copy(pt.ftsp_t.begin(), pt.ftsp_t.end(), tt.begin() + (size_t)p * rows);
        if (!sweep) { std::copy(pt.tailx.begin(), pt.tailx.end(), tx.begin() + p * nm); std::copy(pt.taily.begin(), pt.taily.end(), ty.begin() + p * nm); }
    }
    const int rc = upload_all(h, h->pl_midx, &pl.midx, h->pl_midy, &pl.midy, mxy, &pl.midxy, tt, &pl.t);
    return (rc != ISMPC_OK || sweep) ? rc : upload_all(h, tx, &pl.tailx, ty, &pl.taily);
}
// ... part 2: one record per (set, plan) pair, set-major -- the set's record (`base`) with the plan's tables in place of plan 0's
std::vector<DevConst> pair_records(const ismpc_handle* h, const std::vector<DevConst>& base, const PlanSlabs& pl)
{
    const int P = h->nplans;
    const size_t nm = (size_t)h->t.nmid, rows = (size_t)h->t.rows;
    std::vector<DevConst> pr(base.size() * (size_t)P);
    for (size_t k = 0; k < base.size(); ++k)
        for (int p = 0; p < P; ++p) {
            DevConst& d = pr[k * P + p]; d = base[k];
            d.midx = pl.midx + p * nm; d.midy = pl.midy + p * nm; d.midxy = pl.midxy + 2 * p * nm; d.ftsp_t = pl.t + p * rows;
            if (h->sweep) { d.tailx = h->sw.tailx + (k * P + p) * h->sw.s_tail; d.taily = h->sw.taily + (k * P + p) * h->sw.s_tail; }
            else { d.tailx = pl.tailx + p * nm; d.taily = pl.taily + p * nm; }
            d.sets = nullptr; d.nsets = 0; d.nplans = 0; d.order = nullptr;
        }
    return pr;
}
// One DevConst record per set of a sweep: the handle's, with the set's scalars and device-built table pointers in place of set 0's host-built ones
std::vector<DevConst> sweep_records(const ismpc_handle* h, const ismpc_params* params, int K)
{
    std::vector<DevConst> cs((size_t)K, h->c);
    for (int k = 0; k < K; ++k) {
        DevConst& d = cs[k]; const ismpc_params& q = params[k];
        const double eta = std::sqrt(q.g / q.h_des);
        d.mass = q.mass; d.h_des = q.h_des; d.half_run = q.foot_width / 2; d.half_first = q.first_step_halfwidth;
        d.q_p = q.q_p; d.q_u = q.q_u; d.q_v = q.q_v; d.z_lo = q.z_ineq_lo; d.z_hi = q.z_ineq_hi; d.eta = eta;
        d.inv_mass = 1.0 / q.mass; d.dt_over_mass = q.mpc_dt / q.mass; d.inv_eta = 1.0 / eta;
        d.vtab = h->sw.vtab + (size_t)k * h->sw.s_vtab; d.vqT = h->sw.vqT + (size_t)k * h->sw.s_vqT;
        d.Wt = h->sw.Wt + (size_t)k * h->sw.s_W; d.SW = h->sw.SW + (size_t)k * h->sw.s_W;
        d.HSt = h->sw.HSt + (size_t)k * h->sw.s_HS; d.SHSt = h->sw.SHSt + (size_t)k * h->sw.s_HS;
        if (h->sw.dU) { d.dU = h->sw.dU + (size_t)k * h->sw.s_dU; d.SdU = h->sw.SdU + (size_t)k * h->sw.s_dU; }      // (plans with mid_z != 0)
        d.tailx = h->sw.tailx + (size_t)k * h->plans() * h->sw.s_tail; d.taily = h->sw.taily + (size_t)k * h->plans() * h->sw.s_tail;
        d.Hinv = nullptr; d.W = nullptr; d.vq = nullptr; d.sets = nullptr; d.nsets = 0;
    }
    return cs;
}

}  // namespace

extern "C" {

int ismpc_abi_version(void) { return ISMPC_ABI_VERSION; }
const char* ismpc_last_error(void) { return g_err.c_str(); }

void ismpc_params_default(ismpc_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->mpc_dt = 0.01; p->control_dt = 0.01;                 // parameters.cpp:9-10
    const double ss = 0.35, ds = 0.1, pred = 1.0;           // parameters.cpp:11-13
    p->N = (int)std::lround(pred / p->mpc_dt);              // :42
    p->S = (int)std::lround(ss / p->mpc_dt);                // :43
    p->F = (int)std::lround(ds / p->mpc_dt);                // :44
    p->M = 2;                                               // :45
    p->mass = 50.0; p->g = 9.81; p->h_des = 0.69;           // :39,40,16
    p->foot_width = 0.09; p->first_step_halfwidth = 1.0;    // :21 ; MPCSolver.cpp:334-337
    p->q_p = 1005000.0; p->q_u = 0.01; p->q_v = 100.0;      // MPCSolver.cpp:253-255
    p->z_ineq_lo = 0.0; p->z_ineq_hi = 10000.0;             // MPCSolver.cpp:159-160
    p->lambda_gate = 2.0;                                   // MPCSolver.cpp:322
}

// P: footstep plans of a multi-plan handle (ftsp: P x rows x 4; the handle's own tables come from plan 0), 0 for every other handle
static int create_impl(const ismpc_params* params, int K, bool sweep, const double* ftsp, int rows, int device, ismpc_handle** out, int P = 0)
{
    if (!params || !ftsp || !out) return fail(ISMPC_E_INVALID, "null argument");
    *out = nullptr;
    const Knobs knobs = read_knobs();
    int rc = check_args(params, K, sweep, ftsp, rows, P, knobs);
    if (rc != ISMPC_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(ISMPC_E_NO_DEVICE, "no HIP device visible: the ISMPC hot path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(ISMPC_E_INVALID, "device ordinal out of range");
    // the handle is destroyed on every way out but the last
    std::unique_ptr<ismpc_handle, void (*)(ismpc_handle*)> owner(new (std::nothrow) ismpc_handle(), ismpc_destroy);
    ismpc_handle* h = owner.get();
    if (!h) return fail(ISMPC_E_ALLOC, "out of host memory");
    h->device = device;
    std::string err;
    rc = ismpc::build_tables(*params, ftsp, rows, h->t, err);
    if (rc != ISMPC_OK) return fail(rc, err);
    h->force_waves = knobs.force_waves; h->dense_path = knobs.dense; h->quad_path = !knobs.dense && !knobs.wave;
    h->z_fallback = knobs.z_fallback; h->kernel_rollout = knobs.kernel_rollout; h->one_launch = knobs.one_launch; h->host_mode = knobs.host_mode;
    if (knobs.lpi) { h->lpi = knobs.lpi; h->lpi_auto = false; }
    h->nplans = P;
    if (sweep) {      // one kernel shape: 16 lanes per instance (ISMPC_Z_FALLBACK=0 still means flag-only: bench.py times the tick kernel alone with it)
        h->sweep = true; h->lpi = 16; h->lpi_auto = false; h->quad_path = true; h->dense_path = false;
        h->sets.assign(params, params + K); h->ftsp.assign(ftsp, ftsp + (size_t)rows * 4);
    }
    DeviceGuard guard_(device);
    if (guard_.err != hipSuccess) return fail(ISMPC_E_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(guard_.err));
    { hipDeviceProp_t prop; h->cus = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 0; }
    fill_constants(h->t, knobs.zldsq, h->c);
    rc = upload_tables(h, h->lpi_auto || sweep);
    if (rc != ISMPC_OK) return rc;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess ||
        hipEventCreate(&h->ev1) != hipSuccess) return fail(ISMPC_E_NO_DEVICE, "stream/event creation failed");
    PlanSlabs pl;
    if (P) rc = upload_plans(h, params[0], ftsp, pl);
    if (rc != ISMPC_OK) return rc;
    // the records c.sets points to: per set for a sweep, per (set, plan) pair for a multi-plan handle
    auto records = [&](const std::vector<DevConst>& base) { return P ? pair_records(h, base, pl) : base; };
    const char* what = P ? "multi-plan handle" : "sweep";
    const DevConst* recs = nullptr;
    if (sweep) {
        // every set's tables, built on the device (MFMA Newton-Schulz inverse of the K vertical Hessians, csrc/ismpc_sweep.hip)
        std::string serr;
        // 8 lanes per instance beyond LPI16_BATCH, as plain handles take them (ISMPC_LPI=16 keeps 16 at every size).  With eight instances
        // of a wavefront reading eight sets' tables it measured level to 2 % slower on the 64-set batch (round 3: 9.25-9.28 against
        // 9.27-9.43e8 ticks/s); with the batch sorted by set (ismpc_sweep_bind: one set per wavefront) it is 5 % faster (round 4: 9.65-9.71
        // against 9.17-9.26e8), so it is the default now
        const bool lanes8 = knobs.lpi != 16;
        rc = ismpc::sweep_build(params, K, h->t, P ? pl.midx : h->c.midx, P ? pl.midy : h->c.midy, h->c.midz, h->c.e_lo, h->c.ne, 16, quad_R(h->c.N, 16), lanes8 ? 8 : 0, quad_R(h->c.N, 8),
                                h->own_stream, h->sw, h->dev_allocs, serr, h->plans());
        if (rc != ISMPC_OK) return fail(rc, serr);
        // the set records over the 16-lane copy of the affine tables and, beside them, over the 8-lane copy (pick_layout)
        std::vector<DevConst> cs = sweep_records(h, params, K);
        rc = upload_records(h, records(cs), &recs, what);
        if (rc == ISMPC_OK && h->sw.vqT2) {
            for (int k = 0; k < K; ++k) cs[k].vqT = h->sw.vqT2 + (size_t)k * h->sw.s_vqT2;
            rc = upload_records(h, records(cs), &h->sets8, what);
        }
    } else if (P) {
        // one parameter set: the pair records are the handle's own constants per plan, once per lane layout it may launch with
        std::vector<DevConst> base(1, h->c);
        rc = upload_records(h, records(base), &recs, what);
        if (rc == ISMPC_OK && h->vqT32) { base[0].vqT = h->vqT32; rc = upload_records(h, records(base), &h->sets32, what); }
        if (rc == ISMPC_OK && h->vqT8) { base[0].vqT = h->vqT8; rc = upload_records(h, records(base), &h->sets8, what); }
    }
    if (rc != ISMPC_OK) return rc;
    if (recs) { h->c.sets = recs; h->c.nsets = K; h->c.nplans = P; }
    // the constants in device memory, last: with everything above in them
    rc = upload_records(h, std::vector<DevConst>(1, h->c), &h->c_dev, "constants");
    if (rc != ISMPC_OK) return rc;
    *out = owner.release();
    return ISMPC_OK;
}

int ismpc_create(const ismpc_params* params, const double* ftsp, int rows, int device, ismpc_handle** out)
{
    return create_impl(params, 1, false, ftsp, rows, device, out);
}

int ismpc_create_sweep(const ismpc_params* params, int n_sets, const double* ftsp, int rows, int device, ismpc_handle** out)
{
    return create_impl(params, n_sets, true, ftsp, rows, device, out);
}

int ismpc_create_plans(const ismpc_params* params, int n_sets, const double* ftsp, int n_plans, int rows, int device, ismpc_handle** out)
{
    if (n_plans < 1) return fail(ISMPC_E_INVALID, "a multi-plan handle holds 1 .. 32767 footstep plans");
    return create_impl(params, n_sets, n_sets > 1, ftsp, rows, device, out, n_plans);
}

int ismpc_plans_info(const ismpc_handle* h, int* n_plans)
{
    if (!h || !n_plans) return fail(ISMPC_E_INVALID, "null argument");
    *n_plans = h->plans();
    return ISMPC_OK;
}

int ismpc_get_midpoint_plan(const ismpc_handle* h, int plan, double* dst, int capacity_rows)
{
    if (!h || !dst || capacity_rows < h->t.nmid || plan < 0 || plan >= h->plans()) return fail(ISMPC_E_INVALID, "bad argument");
    if (!h->nplans) return ismpc_get_midpoint(h, dst, capacity_rows);
    const size_t o = (size_t)plan * h->t.nmid;
    for (int i = 0; i < h->t.nmid; ++i) { dst[3*i] = h->pl_midx[o + i]; dst[3*i+1] = h->pl_midy[o + i]; dst[3*i+2] = h->t.midz[i]; }
    return ISMPC_OK;
}

int ismpc_sweep_bind(ismpc_handle* h, int batch, const ismpc_tick_in* in_dev, void* stream)
{
    if (!h || batch < 0 || (batch > 0 && !in_dev)) return fail(ISMPC_E_INVALID, "bad argument");
    if (!h->sweep && !h->nplans) return fail(ISMPC_E_INVALID, "ismpc_sweep_bind needs a handle of ismpc_create_sweep or ismpc_create_plans");
    ON_DEVICE(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (batch == 0) { h->order_batch = 0; return ISMPC_OK; }
    const int nb = h->c.nsets * h->plans() + 1;      // (a multi-plan handle sorts by (set, plan) pair)
    if (batch + nb > h->order_cap) {
        HIP_TRY(hipDeviceSynchronize());                       // (a set-up call: launches that still read the old order finish first)
        h->order_batch = 0;
        ISMPC_GROW_SYNC(fail, h->order, h->order_cap, batch + nb, sizeof(int) * (size_t)(batch + nb));
    }
    int* cursor = h->order + batch;
    HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(int) * (size_t)nb, s));
    const dim3 grid((batch + 255) / 256), block(256);
    with_sw(h, [&](auto SW) {
        if constexpr (SW != 0) {                     // (neither a sweep nor a multi-plan handle: refused above)
            hipLaunchKernelGGL(sweep_sort_hist<SW>, grid, block, 0, s, h->c, in_dev, batch, cursor);
            hipLaunchKernelGGL(sweep_sort_scan, dim3(1), block, 0, s, cursor, nb);
            hipLaunchKernelGGL(sweep_sort_scatter<SW>, grid, block, 0, s, h->c, in_dev, batch, cursor, h->order);
        }
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    h->order_batch = batch;
    return ISMPC_OK;
}

int ismpc_sweep_info(const ismpc_handle* h, int* n_sets, int* newton_iterations, int* mfma_gemm_launches, double* build_ms)
{
    if (!h) return fail(ISMPC_E_INVALID, "null handle");
    if (n_sets) *n_sets = h->sweep ? h->sw.K : 1;
    if (newton_iterations) *newton_iterations = h->sweep ? h->sw.newton_iters : 0;
    if (mfma_gemm_launches) *mfma_gemm_launches = h->sweep ? h->sw.gemm_launches : 0;
    if (build_ms) *build_ms = h->sweep ? (double)h->sw.build_ms : 0.0;
    return ISMPC_OK;
}

// The device-built tables of one set against the host's long-double build of the same parameters (csrc/ismpc_tables.cpp):
// rel_err[t] = max |device - host| / max |host| for t = 0 H^-1, 1 affine tables (U0,Ua,Ub,SU0,SUa,SUb per pattern), 2 W_p, 3 S W_p,
// 4 Hinv S', 5 S Hinv S', 6 anticipative tails, 7 lane-group layout of the affine tables.
int ismpc_sweep_verify_tables(ismpc_handle* h, int set, double* rel_err)
{
    if (!h || !rel_err) return fail(ISMPC_E_INVALID, "null argument");
    if (!h->sweep || set < 0 || set >= h->sw.K) return fail(ISMPC_E_INVALID, "not a sweep handle, or set out of range");
    ON_DEVICE(h);
    ismpc::Tables t; std::string err;
    int rc = ismpc::build_tables(h->sets[set], h->ftsp.data(), h->t.rows, t, err);
    if (rc != ISMPC_OK) return fail(rc, err);
    const ismpc::SweepSlabs& S = h->sw;
    const int N = t.p.N, NG = S.NG;
    auto fetch = [&](const double* src, size_t n, std::vector<double>& dst) -> bool { dst.resize(n); return hipMemcpy(dst.data(), src, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess; };
    auto rel = [](const std::vector<double>& d, const std::vector<double>& hst) { double e = 0, m = 0; for (size_t i = 0; i < hst.size(); ++i) { e = std::max(e, std::fabs(d[i] - hst[i])); m = std::max(m, std::fabs(hst[i])); } return m > 0 ? e / m : e; };
    std::vector<double> d, hv;
    if (!fetch(S.X0 + (size_t)set * S.s_mat, S.s_mat, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
    { std::vector<double> a((size_t)N * N), b((size_t)N * N); for (int i = 0; i < N; ++i) for (int j = 0; j < N; ++j) { a[(size_t)i*N+j] = d[(size_t)i*NG+j]; b[(size_t)i*N+j] = t.Hinv[(size_t)i*t.NP+j]; } rel_err[0] = rel(a, b); }
    if (!fetch(S.vtab + (size_t)set * S.s_vtab, S.s_vtab, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
    rel_err[1] = rel(d, t.vtab);
    if (!fetch(S.Wt + (size_t)set * S.s_W, S.s_W, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
    rel_err[2] = rel(d, t.Wt);
    if (!fetch(S.SW + (size_t)set * S.s_W, S.s_W, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
    rel_err[3] = rel(d, t.SW);
    if (!fetch(S.HSt + (size_t)set * S.s_HS, S.s_HS, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
    rel_err[4] = rel(d, t.HSt);
    if (!fetch(S.SHSt + (size_t)set * S.s_HS, S.s_HS, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
    rel_err[5] = rel(d, t.SHSt);
    { std::vector<double> dx, dy; const size_t ts = (size_t)set * h->plans() * S.s_tail;      // (a multi-plan handle: the tails of (set, plan 0))
      if (!fetch(S.tailx + ts, S.s_tail, dx) || !fetch(S.taily + ts, S.s_tail, dy)) return fail(ISMPC_E_NO_DEVICE, "download failed");
      rel_err[6] = std::max(rel(dx, t.tailx), rel(dy, t.taily)); }
    rel_err[7] = 0.0;
    for (int pass = 0; pass < (S.vqT2 ? 2 : 1); ++pass) {   // the lane-group layouts (16 lanes, 8 lanes), against the host's re-striding of ITS vtab
        const int lpi = pass == 0 ? 16 : 8;
        std::vector<double> tzgT;
        ismpc::lane_group_tables(t, lpi, quad_R(N, lpi), hv, tzgT);
        if (!fetch(pass == 0 ? S.vqT + (size_t)set * S.s_vqT : S.vqT2 + (size_t)set * S.s_vqT2, pass == 0 ? S.s_vqT : S.s_vqT2, d)) return fail(ISMPC_E_NO_DEVICE, "download failed");
        rel_err[7] = std::max(rel_err[7], rel(d, hv));
    }
    return ISMPC_OK;
}

void ismpc_destroy(ismpc_handle* h)
{
    if (!h) return;
    DeviceGuard guard_(h->device);
    for (void* p : h->dev_allocs) (void)hipFree(p);
    if (h->st_in) (void)hipFree(h->st_in);
    if (h->st_out) (void)hipFree(h->st_out);
    if (h->zseen_host) (void)hipHostFree(h->zseen_host);
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    if (h->zmark) (void)hipFree(h->zmark);
    if (h->order) (void)hipFree(h->order);
    if (h->zstop) (void)hipFree(h->zstop);
    if (h->mcrec) (void)hipFree(h->mcrec);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int ismpc_solve_batch_device(ismpc_handle* h, int batch, const ismpc_tick_in* in_dev, ismpc_tick_out* out_dev,
                             double* u_traj, void* stream)
{
    if (!h || batch < 0 || (batch > 0 && (!in_dev || !out_dev))) return fail(ISMPC_E_INVALID, "bad argument");
    ON_DEVICE(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h->timing) HIP_TRY(hipEventRecord(h->ev0, s));
    int rc = launch(h, batch, in_dev, nullptr, out_dev, u_traj, -1, s);
    if (rc != ISMPC_OK) return rc;
    if (h->timing) { HIP_TRY(hipEventRecord(h->ev1, s)); h->timed_pending = true; }
    return ISMPC_OK;
}

int ismpc_solve_batch(ismpc_handle* h, int batch, const ismpc_tick_in* in_host, ismpc_tick_out* out_host)
{
    if (!h || batch < 0 || (batch > 0 && (!in_host || !out_host))) return fail(ISMPC_E_INVALID, "bad argument");
    if (batch == 0) return ISMPC_OK;
    ON_DEVICE(h);
    // A batch of a few instances (the reference's own call: one MPCSolver::solve per control tick) is all latency: the kernel
    // reads its records from, and writes them to, host memory mapped into the device's address space -- two memcpy submissions
    // less than the staged path below.  ISMPC_PINNED=0 switches it off.
    constexpr int PIN_BATCH = 64;
    if (batch <= PIN_BATCH && !h->pin_off) {
        if (!h->pin_in) {
            if (const char* e = std::getenv("ISMPC_PINNED")) h->pin_off = std::atoi(e) == 0;
            if (!h->pin_off) {
                if (hipHostMalloc((void**)&h->pin_in, sizeof(ismpc_tick_in) * PIN_BATCH, hipHostMallocMapped) != hipSuccess ||
                    hipHostMalloc((void**)&h->pin_out, sizeof(ismpc_tick_out) * PIN_BATCH, hipHostMallocMapped) != hipSuccess) {
                    (void)hipGetLastError(); h->pin_off = true;
                    if (h->pin_in) { (void)hipHostFree(h->pin_in); h->pin_in = nullptr; }
                }
            }
        }
        if (!h->pin_off) {
            ismpc_tick_in* din = nullptr; ismpc_tick_out* dout = nullptr;
            HIP_TRY(hipHostGetDevicePointer((void**)&din, h->pin_in, 0));
            HIP_TRY(hipHostGetDevicePointer((void**)&dout, h->pin_out, 0));
            std::memcpy(h->pin_in, in_host, sizeof(ismpc_tick_in) * (size_t)batch);
            const int rc = ismpc_solve_batch_device(h, batch, din, dout, nullptr, h->own_stream);
            if (rc != ISMPC_OK) return rc;
            HIP_TRY(hipStreamSynchronize(h->own_stream));
            std::memcpy(out_host, h->pin_out, sizeof(ismpc_tick_out) * (size_t)batch);
            return ISMPC_OK;
        }
    }
    // zero copy needs device-visible addresses for the caller's records (page-locked AND mapped: hipHostMalloc / hipHostRegister give
    // both under unified addressing); anything else -- also a registration without a device mapping -- takes the staged path
    const ismpc_tick_in* zc_in = nullptr; ismpc_tick_out* zc_out = nullptr;
    bool zero_copy = h->host_mode != 0 && !h->dense_path && host_is_pinned(in_host, sizeof(ismpc_tick_in) * (size_t)batch) && host_is_pinned(out_host, sizeof(ismpc_tick_out) * (size_t)batch);
    if (zero_copy && (hipHostGetDevicePointer((void**)&zc_in, const_cast<ismpc_tick_in*>(in_host), 0) != hipSuccess ||
                      hipHostGetDevicePointer((void**)&zc_out, out_host, 0) != hipSuccess)) { (void)hipGetLastError(); zero_copy = false; }
    if (batch > h->st_cap && !(zero_copy && h->host_mode == 3)) {      // device staging (not needed when both sides are in place)
        if (h->st_in) (void)hipFree(h->st_in);
        if (h->st_out) (void)hipFree(h->st_out);
        h->st_in = nullptr; h->st_out = nullptr; h->st_cap = 0;
        HIP_TRY(hipMalloc((void**)&h->st_in, sizeof(ismpc_tick_in) * (size_t)batch));
        HIP_TRY(hipMalloc((void**)&h->st_out, sizeof(ismpc_tick_out) * (size_t)batch));
        h->st_cap = batch;
    }
    // Page-locked caller buffers (hipHostMalloc / hipHostRegister / ismpc_host_alloc / ismpc_host_register): ZERO COPY -- the kernel
    // reads the records from, and writes them to, the caller's memory over PCIe.  Reads and writes travel in opposite directions
    // at the same time and no DMA submission sits in front of or behind the launch.  Measured on MI355X at 65 536 records (4.7 MB
    // in, 5.2 MB out; scripts/host_path_probe.py): 0.193 ms per call against 0.257 ms for DMA in -> kernel -> DMA out from the same
    // buffers; chunking that pipeline over two streams gains nothing (0.243 ms with 2 chunks, slower with more: each DMA
    // submission costs ~10 us), nor do non-coherent / write-combined allocations or 64-byte-line stores.  ISMPC_HOST_MODE: bit 0 =
    // read in place, bit 1 = write in place (default 3; 0 = the staged path).  Same kernel, same records, bit for bit.
    // Pageable buffers take the staged path below (the HIP runtime stages them).
    if (zero_copy) {
        const ismpc_tick_in* din = h->st_in; ismpc_tick_out* dout = h->st_out;
        hipStream_t s = h->own_stream;
        if (h->host_mode & 1) din = zc_in;
        else HIP_TRY(hipMemcpyAsync(h->st_in, in_host, sizeof(ismpc_tick_in) * (size_t)batch, hipMemcpyHostToDevice, s));
        if (h->host_mode & 2) dout = zc_out;
        const int rc = ismpc_solve_batch_device(h, batch, din, dout, nullptr, s);
        if (rc != ISMPC_OK) return rc;
        if (!(h->host_mode & 2)) HIP_TRY(hipMemcpyAsync(out_host, h->st_out, sizeof(ismpc_tick_out) * (size_t)batch, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return ISMPC_OK;
    }
    hipStream_t s = h->own_stream;
    HIP_TRY(hipMemcpyAsync(h->st_in, in_host, sizeof(ismpc_tick_in) * (size_t)batch, hipMemcpyHostToDevice, s));
    int rc = ismpc_solve_batch_device(h, batch, h->st_in, h->st_out, nullptr, s);
    if (rc != ISMPC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_host, h->st_out, sizeof(ismpc_tick_out) * (size_t)batch, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ISMPC_OK;
}

// The closed loop of ismpc_rollout_device and of ismpc_rollout_mc_device (mc = true: pushes, trajectory stride, summaries): ONE host launch
// function for both, in the kernel (ismpc_rollout_quad, MC = mc) where the handle runs its loops there, one launch per tick otherwise.
static int rollout_impl(ismpc_handle* h, int batch, ismpc_tick_in* state_dev, int first_frame, int ticks, bool mc, const ismpc_push* pushes_dev,
                        int n_push, int traj_stride, ismpc_tick_out* traj_dev, ismpc_rollout_summary* summary_dev, hipStream_t s)
{
    ON_DEVICE(h);
    StreamMark mark_{h, s};
    if (h->timing) HIP_TRY(hipEventRecord(h->ev0, s));
    // the scratch record per instance: where a tick leaves its record for the summary and the resume launch its fallback ticks
    if (mc && batch > h->mcrec_cap)              // stream-ordered growth, as zmark (ismpc_reserve sizes it beforehand)
        ISMPC_GROW_ASYNC(fail, h, h->mcrec, h->mcrec_cap, batch, sizeof(ismpc_tick_out) * (size_t)batch, s);
    if (batch > 0 && ticks > 0 && h->kernel_rollout && !h->dense_path && h->quad_path && h->c.N <= 128 && h->z_fallback) {
        // the whole closed loop in ONE launch: state in registers, one trajectory record per tick (ismpc_rollout_quad)
        const QuadLaunch q = quad_launch(h, batch, false);
        if (batch > h->zstop_cap)                         // stream-ordered growth, as zmark (ismpc_reserve sizes it beforehand)
            ISMPC_GROW_ASYNC(fail, h, h->zstop, h->zstop_cap, batch, sizeof(int) * (size_t)batch, s);
        const int lid = ++h->launch_id;
        const dim3 rgrid(std::min((batch + ISMPC_QUAD_WAVES - 1) / ISMPC_QUAD_WAVES, 64));
        const RolloutMc m{pushes_dev, n_push, traj_stride, summary_dev, h->mcrec};
        auto both = [&](auto MC_) {
            constexpr bool MCv = decltype(MC_)::value;
            return with_sw(h, [&](auto SW) {
                constexpr int sw = decltype(SW)::value;
                return quad_shape(h->c.N, q.lpi, [&](auto RR, auto LL, auto RW_) {
                    if constexpr (has_rollout_quad(LL, sw)) {
                        // the rollout itself, then its resume launch (FB = true)
                        hipLaunchKernelGGL((ismpc_rollout_quad<RR, LL, RW_, false, sw, MCv>), q.grid, q.block, 0, s, q.c, state_dev, traj_dev, batch, first_frame, ticks, h->zstop, lid, m);
                        hipLaunchKernelGGL((ismpc_rollout_quad<RR, LL, RW_, true, sw, MCv>), rgrid, q.block, 0, s, q.c, state_dev, traj_dev, batch, first_frame, ticks, h->zstop, lid, m);
                        const int v[8] = {ISMPC_KERNEL_ROLLOUT_QUAD, LL, RR, RW_, form_bits(h) | (MCv ? 4 : 0), 2, batch, 0};      // (ismpc_last_launch_info: the rollout and its resume launch)
                        std::memcpy(h->last_launch, v, sizeof(v));
                        return ISMPC_OK;
                    } else      // (a sweep handle rolls out at 16 lanes per instance: the SW = 1 kernels are instantiated for that shape only)
                        return fail(ISMPC_E_UNSUPPORTED, "parameter sweep: rollouts take 16 lanes per instance");
                });
            });
        };
        const int rc = mc ? both(std::true_type{}) : both(std::false_type{});
        if (rc != ISMPC_OK) return rc;
        HIP_TRY(hipGetLastError());
    } else {
        // one launch per tick; the disturbed form puts its two elementwise kernels around it and chooses the trajectory row here
        const dim3 egrid((batch + 255) / 256), eblock(256);
        if (summary_dev && batch > 0) hipLaunchKernelGGL(ismpc_mc_fold, egrid, eblock, 0, s, nullptr, batch, summary_dev, 0);      // (the empty summary)
        for (int t = 0; t < ticks; ++t) {
            if (n_push > 0 && batch > 0) hipLaunchKernelGGL(ismpc_mc_push, egrid, eblock, 0, s, state_dev, batch, pushes_dev, n_push, t);
            const bool rec_t = (t + 1) % traj_stride == 0;
            ismpc_tick_out* out = (rec_t && traj_dev) ? traj_dev + (size_t)((t + 1) / traj_stride - 1) * batch : (summary_dev ? h->mcrec : nullptr);
            int rc = launch(h, batch, nullptr, state_dev, out, nullptr, first_frame + t, s);
            if (rc != ISMPC_OK) return rc;
            if (summary_dev && batch > 0) hipLaunchKernelGGL(ismpc_mc_fold, egrid, eblock, 0, s, out, batch, summary_dev, t);
        }
        if (mc) HIP_TRY(hipGetLastError());
    }
    if (h->timing) { HIP_TRY(hipEventRecord(h->ev1, s)); h->timed_pending = true; }
    return ISMPC_OK;
}

int ismpc_rollout_device(ismpc_handle* h, int batch, ismpc_tick_in* state_dev, int first_frame, int ticks,
                         ismpc_tick_out* traj_dev, void* stream)
{
    if (!h || batch < 0 || ticks < 0 || first_frame < 0 || (batch > 0 && !state_dev)) return fail(ISMPC_E_INVALID, "bad argument");
    return rollout_impl(h, batch, state_dev, first_frame, ticks, false, nullptr, 0, 1, traj_dev, nullptr, static_cast<hipStream_t>(stream));
}

int ismpc_rollout_mc_device(ismpc_handle* h, int batch, ismpc_tick_in* state_dev, int first_frame, int ticks,
                            const ismpc_push* pushes_dev, int n_push, int traj_stride, ismpc_tick_out* traj_dev,
                            ismpc_rollout_summary* summary_dev, void* stream)
{
    // (what can be said about the numbers is said first: each message is reachable without a handle, i.e. without a device)
    if (batch < 0 || ticks < 0 || first_frame < 0) return fail(ISMPC_E_INVALID, "ismpc_rollout_mc_device: negative batch, ticks or first_frame");
    if (traj_stride < 1) return fail(ISMPC_E_INVALID, "ismpc_rollout_mc_device: traj_stride must be at least 1");
    if (n_push < 0) return fail(ISMPC_E_INVALID, "ismpc_rollout_mc_device: negative n_push");
    if (n_push > 0 && !pushes_dev) return fail(ISMPC_E_INVALID, "ismpc_rollout_mc_device: n_push > 0 with a null push table");
    if (!h) return fail(ISMPC_E_INVALID, "ismpc_rollout_mc_device: null handle");
    if (batch > 0 && !state_dev) return fail(ISMPC_E_INVALID, "ismpc_rollout_mc_device: null state");
    return rollout_impl(h, batch, state_dev, first_frame, ticks, true, pushes_dev, n_push, traj_stride, traj_dev, summary_dev, static_cast<hipStream_t>(stream));
}

// Page-locked host memory for callers without HIP headers (the pipelined ismpc_solve_batch needs it on both sides).
int ismpc_host_alloc(size_t bytes, void** out)
{
    if (!out || bytes == 0) return fail(ISMPC_E_INVALID, "bad argument");
    *out = nullptr;
    unsigned flags = hipHostMallocDefault;
    if (const char* e = std::getenv("ISMPC_HOST_ALLOC_FLAGS")) flags = (unsigned)std::strtoul(e, nullptr, 0);
    if (hipHostMalloc(out, bytes, flags) != hipSuccess) { (void)hipGetLastError(); return fail(ISMPC_E_ALLOC, "hipHostMalloc failed"); }
    return ISMPC_OK;
}
int ismpc_host_free(void* p)
{
    if (!p) return ISMPC_OK;
    HIP_TRY(hipHostFree(p));
    return ISMPC_OK;
}
int ismpc_host_register(void* p, size_t bytes)
{
    if (!p || bytes == 0) return fail(ISMPC_E_INVALID, "bad argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return ISMPC_OK;
}
int ismpc_host_unregister(void* p)
{
    if (!p) return fail(ISMPC_E_INVALID, "bad argument");
    HIP_TRY(hipHostUnregister(p));
    return ISMPC_OK;
}

int ismpc_reserve(ismpc_handle* h, int max_batch)
{
    if (!h || max_batch < 0) return fail(ISMPC_E_INVALID, "bad argument");
    ON_DEVICE(h);
    if (h->z_fallback && max_batch > h->zmark_cap) ISMPC_GROW_SYNC(fail, h->zmark, h->zmark_cap, max_batch, zscratch_bytes(max_batch));
    if (max_batch > h->zstop_cap) ISMPC_GROW_SYNC(fail, h->zstop, h->zstop_cap, max_batch, sizeof(int) * (size_t)max_batch);
    if (max_batch > h->mcrec_cap) ISMPC_GROW_SYNC(fail, h->mcrec, h->mcrec_cap, max_batch, sizeof(ismpc_tick_out) * (size_t)max_batch);
    return ISMPC_OK;
}

#ifdef ISMPC_STAMPS
int ismpc_debug_stamps(unsigned long long* dst, int reset)
{
    if (dst && hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 16384 * 8) != hipSuccess) return -2;
    if (reset) { std::vector<unsigned long long> z(16384 * 8, 0ull); if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z.data(), z.size() * 8) != hipSuccess) return -2; }
    return 0;
}
#endif

int ismpc_last_launch_info(const ismpc_handle* h, int* out8)
{
    if (!h || !out8) return fail(ISMPC_E_INVALID, "null argument");
    std::memcpy(out8, h->last_launch, sizeof(h->last_launch));
    return ISMPC_OK;
}

int ismpc_fallback_counters(ismpc_handle* h, int* out4)
{
    if (!h || !out4) return fail(ISMPC_E_INVALID, "null argument");
    ON_DEVICE(h);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out4, h->c.zflag, 4 * sizeof(int), hipMemcpyDeviceToHost));
    return ISMPC_OK;
}

int ismpc_get_params(const ismpc_handle* h, ismpc_params* out)
{
    if (!h || !out) return fail(ISMPC_E_INVALID, "null argument");
    *out = h->t.p; return ISMPC_OK;
}
int ismpc_midpoint_rows(const ismpc_handle* h) { return h ? h->t.nmid : ISMPC_E_INVALID; }
int ismpc_get_midpoint(const ismpc_handle* h, double* dst, int capacity_rows)
{
    if (!h || !dst || capacity_rows < h->t.nmid) return fail(ISMPC_E_INVALID, "bad argument");
    for (int i = 0; i < h->t.nmid; ++i) { dst[3*i] = h->t.midx[i]; dst[3*i+1] = h->t.midy[i]; dst[3*i+2] = h->t.midz[i]; }
    return ISMPC_OK;
}
int ismpc_set_timing(ismpc_handle* h, int enabled)
{
    if (!h) return fail(ISMPC_E_INVALID, "null handle");
    h->timing = enabled != 0; h->timed_pending = false; return ISMPC_OK;
}
double ismpc_last_kernel_ms(ismpc_handle* h)
{
    if (!h || !h->timing) return 0.0;
    if (h->timed_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(h->ev1) == hipSuccess && hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_ms = ms;
        h->timed_pending = false;
    }
    return h->last_ms;
}

}  // extern "C"
