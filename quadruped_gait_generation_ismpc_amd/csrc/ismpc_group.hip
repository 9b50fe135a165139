// Multi-GPU layer of the C ABI (include/ismpc_group.h): contiguous shards of a batch of independent gait instances, one
// handle + launch stream + side stream per device, and the path's one collective -- the all-gather of the 80-byte output
// records -- on RCCL.  Host C++ around the single-device entry points of include/ismpc.h / include/ismpc_a.h, called once per local
// device, and ONE kernel of its own: records_to_instance_major, which turns a rollout's tick-major trajectory into the instance-major
// block a shard is in the gathered trajectory.
//
// Reference: Controller.cpp:105-106 constructs ONE MPCSolver and :346-348 calls it from one thread; there is no
// multi-device code in the reference to follow.  Layout per device (HBM):
//     d_all[2]   gathered output records of a step (batch x 80 B), two buffers: the kernel of step k writes its shard at
//                offset first_r x 80 of buffer k & 1, the all-gather fills in the other shards IN PLACE
//     d_in       this device's shard of host-given input records (host entry points only)
//     d_stage    a rollout's trajectory as the single-device call writes it (rows x count_l records, tick-major); never handed out
// Stream order per device and buffer b:   launch stream: wait gathered[b] -> kernel -> record computed[b]
//                                         side stream:   wait computed[b] -> ncclAllGather -> record gathered[b]
// A rollout (ismpc_group_rollout_mc_device) is the same chain on a third pair of events (slot ROLL): its outputs are caller-owned,
//     launch stream: wait gathered[ROLL] -> rollout (summary at summary_all + first, trajectory into d_stage)
//                    -> records_to_instance_major (d_stage -> traj_all + first * rows) -> record computed[ROLL]
//     side stream:   wait computed[ROLL] -> one fused group: all-gather of the summaries, all-gather of the trajectories
//                    -> record gathered[ROLL]
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ismpc_group.h"
#include "ismpc_host.hpp"
#include "ismpc_rccl_load.hpp"

namespace {

thread_local std::string g_gerr = "";
int gfail(int code, const std::string& msg) { g_gerr = msg; return code; }
#define G_HIP(expr) ISMPC_HIP_TRY(gfail, expr)

// ---- RCCL, bound at run time ----------------------------------------------------------------------------------------
// A process that already maps a copy of RCCL (a torch process maps torch/lib/librccl.so, which has no SONAME) must not get a
// second one: the copy found in /proc/self/maps is opened by its path; otherwise $ISMPC_RCCL_LIB, then librccl.so.1.
struct Rccl {
    void* lib = nullptr; std::string err, path; bool test_double = false;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
};
Rccl g_rccl; std::once_flag g_rccl_once;

std::string mapped_rccl()
{
    FILE* f = std::fopen("/proc/self/maps", "r");
    if (!f) return "";
    char line[4096]; std::string found;
    while (found.empty() && std::fgets(line, sizeof line, f)) found = ismpc_rccl::maps_line_path(line);
    std::fclose(f);
    return found;
}

void load_rccl()
{
    Rccl& r = g_rccl;
    std::vector<std::string> tries;
    const std::string m = mapped_rccl();
    if (!m.empty()) tries.push_back(m);
    if (const char* e = std::getenv("ISMPC_RCCL_LIB")) tries.push_back(e);
    tries.push_back("librccl.so.1"); tries.push_back("/opt/rocm/lib/librccl.so.1"); tries.push_back("librccl.so");
    const ismpc_rccl::Opened o = ismpc_rccl::open_first(tries);
    r.lib = o.lib; r.path = o.path; r.err = o.error_text();
    if (!r.lib) return;
#define BIND(name) r.name = reinterpret_cast<decltype(r.name)>(dlsym(r.lib, "nccl" #name)); if (!r.name) { r.err = "nccl" #name " missing in " + r.path; r.lib = nullptr; return; }
    BIND(GetUniqueId) BIND(CommInitRank) BIND(CommInitAll) BIND(CommDestroy) BIND(CommCount) BIND(AllGather) BIND(Broadcast)
    BIND(GroupStart) BIND(GroupEnd) BIND(GetErrorString) BIND(GetVersion)
#undef BIND
    // the in-process test double of tests/helpers/fake_rccl.cpp runs several ranks on ONE device; no RCCL exports this symbol
    r.test_double = dlsym(r.lib, "ismpc_test_rccl_double") != nullptr;
}
Rccl* rccl()
{
    std::call_once(g_rccl_once, load_rccl);
    return g_rccl.lib ? &g_rccl : nullptr;
}
#define G_NCCL(expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) \
    return gfail(ISMPC_E_NO_DEVICE, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); } while (0)

struct DevGuard {
    int prev = -1, dev; hipError_t err = hipSuccess;
    explicit DevGuard(int d) : dev(d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) err = hipSetDevice(dev); }
    ~DevGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

void shard(int batch, int rank, int world, int* first, int* count)
{
    const int base = batch / world, extra = batch % world;
    *count = base + (rank < extra ? 1 : 0);
    *first = rank * base + (rank < extra ? rank : extra);
}

// ---- tick-major -> instance-major records ------------------------------------------------------------------------------
// A rollout writes its trajectory [row][instance of the shard]; the gathered trajectory is [instance][row], so that a shard is one
// contiguous block:  dst[i * rows + row] = src[row * count + i], records of 80 bytes = five 16-byte pieces, moved as uint4 on both sides.
// One workgroup moves tiles of PK_TR rows x PK_TI instances through LDS: the loads of a tile are PK_TR runs of PK_TI * 80 contiguous
// bytes (along the instance axis), the stores PK_TI runs of PK_TR * 80 contiguous bytes (along the row axis); one thread per record
// would store 80-byte fragments rows * 80 bytes apart.  LDS image: the tile in SOURCE order, a row every PK_ROW 16-byte slots with
// PK_ROW = 5 (mod 16).  Stores into it are consecutive slots (ds_write_b128: groups of 8 consecutive lanes, 8 slots per bank row of
// 32 dwords, and 8 divides PK_TI * 5, so a group never straddles a row).  The transposed read of piece p of row r of instance i is
// slot r * PK_ROW + 5 i + p = (5 r + p) + 5 i (mod 16): the 16 lanes of a ds_read_b128 group that walk one instance's 5 r + p read
// 16 different slots of the 64-dword bank row.  Tiles are numbered row-tile fastest: neighbouring workgroups store neighbouring runs
// of the same instances, so the cache lines two runs share are completed in L2.
// Tile: 8 rows x 32 instances (loads in runs of 2 560 bytes, stores in runs of 640, a 21 120-byte image); 16 x 16, 32 x 8 and 32 x 16 were
// measured beside it: equal at 200 rows, up to 12 % behind at 20.  -DISMPC_PACK_TR / -DISMPC_PACK_TI build the others.
#ifndef ISMPC_PACK_TI
#define ISMPC_PACK_TI 32
#endif
#ifndef ISMPC_PACK_TR
#define ISMPC_PACK_TR 8
#endif
constexpr int PK_TI = ISMPC_PACK_TI, PK_TR = ISMPC_PACK_TR, PK_THREADS = 256, PK_PIECES = 5;
constexpr int PK_ROW = PK_TI * PK_PIECES + (5 + 16 - (PK_TI * PK_PIECES) % 16) % 16;
constexpr size_t PK_MAX_GRID = 4096;      // workgroups; more tiles than that are walked grid-stride
static_assert((PK_TI * PK_PIECES) % 8 == 0 && PK_ROW % 16 == 5, "LDS image of records_to_instance_major");
static_assert(sizeof(ismpc_tick_out) == 16 * PK_PIECES && sizeof(ismpc_a_out) == 16 * PK_PIECES, "an output record is five 16-byte pieces");

__device__ __forceinline__ void pack_tile(const uint4* __restrict__ src, uint4* __restrict__ dst, uint4* lds,
                                          size_t rows, size_t count, size_t row0, size_t i0, int nr, int ni)
{
    const int in_w = ni * PK_PIECES, out_w = nr * PK_PIECES, n = nr * in_w;
    const uint4* s = src + (row0 * count + i0) * PK_PIECES;
#pragma unroll 5
    for (int q = threadIdx.x; q < n; q += PK_THREADS) {
        const int r = q / in_w, c = q - r * in_w;
        lds[r * PK_ROW + c] = s[(size_t)r * count * PK_PIECES + c];
    }
    __syncthreads();
    uint4* d = dst + (i0 * rows + row0) * PK_PIECES;
#pragma unroll 5
    for (int q = threadIdx.x; q < n; q += PK_THREADS) {
        const int i = q / out_w, e = q - i * out_w, r = e / PK_PIECES, p = e - r * PK_PIECES;
        d[(size_t)i * rows * PK_PIECES + e] = lds[r * PK_ROW + i * PK_PIECES + p];
    }
}

__global__ __launch_bounds__(PK_THREADS) void records_to_instance_major(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                        size_t rows, size_t count, size_t tiles_r, size_t tiles)
{
    __shared__ uint4 lds[PK_TR * PK_ROW];
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t ti = t / tiles_r, tr = t - ti * tiles_r;
        const size_t row0 = tr * PK_TR, i0 = ti * PK_TI;
        const int nr = rows - row0 < (size_t)PK_TR ? (int)(rows - row0) : PK_TR, ni = count - i0 < (size_t)PK_TI ? (int)(count - i0) : PK_TI;
        if (nr == PK_TR && ni == PK_TI) pack_tile(src, dst, lds, rows, count, row0, i0, PK_TR, PK_TI);   // (constant widths: no division)
        else pack_tile(src, dst, lds, rows, count, row0, i0, nr, ni);
        __syncthreads();                  // the next tile overwrites the image
    }
}

int pack_records(const void* tick_major, int rows, int count, void* dst_block, hipStream_t stream)
{
    if (rows < 0 || count < 0) return gfail(ISMPC_E_INVALID, "negative rows or count");
    if (rows == 0 || count == 0) return ISMPC_OK;
    if (!tick_major || !dst_block) return gfail(ISMPC_E_INVALID, "null record buffer");
    if ((reinterpret_cast<uintptr_t>(tick_major) | reinterpret_cast<uintptr_t>(dst_block)) & 15) return gfail(ISMPC_E_INVALID, "record buffers must be 16-byte aligned");
    const size_t tiles_r = ((size_t)rows + PK_TR - 1) / PK_TR, tiles = tiles_r * (((size_t)count + PK_TI - 1) / PK_TI);
    const size_t grid = tiles < PK_MAX_GRID ? tiles : PK_MAX_GRID;
    hipLaunchKernelGGL(records_to_instance_major, dim3((unsigned)grid), dim3(PK_THREADS), 0, stream, static_cast<const uint4*>(tick_major),
                       static_cast<uint4*>(dst_block), (size_t)rows, (size_t)count, tiles_r, tiles);
    G_HIP(hipGetLastError());
    return ISMPC_OK;
}

// ---- what both formulations share: devices, streams, events, the gathered buffers, the communicator -------------------
struct Local {
    int device = 0, rank = 0;
    hipStream_t launch = nullptr, side = nullptr;
    hipEvent_t computed[3] = {nullptr, nullptr, nullptr}, gathered[3] = {nullptr, nullptr, nullptr}, after = nullptr;   // slots 0, 1: d_all[b]; ROLL: a rollout's outputs
    bool gathered_set[3] = {false, false, false};
    ncclComm_t comm = nullptr;
    unsigned char* d_all[2] = {nullptr, nullptr}; int all_cap = 0;     // gathered output records
    void* d_in[4] = {nullptr, nullptr, nullptr, nullptr}; size_t in_cap[4] = {0, 0, 0, 0};   // host entry points: the shard's inputs
    void* d_stage = nullptr; size_t stage_cap = 0;                      // a rollout's tick-major trajectory (bytes)
};
enum { ROLL = 2 };

// One output of a step or a rollout as the collective sees it: base[l] = the gathered buffer on local device l, `bytes` per instance.
struct Part { std::vector<unsigned char*> base; size_t bytes = 0; };

struct Core {
    std::vector<Local> loc;
    int world = 0;              // as RCCL reports it
    size_t rec = 80;            // bytes of an output record (ismpc_tick_out and ismpc_a_out are both 80)

    int init_streams()
    {
        for (Local& l : loc) {
            DevGuard gd(l.device); G_HIP(gd.err);
            G_HIP(hipStreamCreateWithFlags(&l.launch, hipStreamNonBlocking));
            G_HIP(hipStreamCreateWithFlags(&l.side, hipStreamNonBlocking));
            for (int b = 0; b < 3; ++b) {
                G_HIP(hipEventCreateWithFlags(&l.computed[b], hipEventDisableTiming));
                G_HIP(hipEventCreateWithFlags(&l.gathered[b], hipEventDisableTiming));
            }
            G_HIP(hipEventCreateWithFlags(&l.after, hipEventDisableTiming));
        }
        return ISMPC_OK;
    }
    int init_comm_all()
    {
        Rccl* r = rccl();
        if (!r) return gfail(ISMPC_E_NO_DEVICE, "RCCL could not be loaded: " + g_rccl.err);
        std::vector<int> devs; for (Local& l : loc) devs.push_back(l.device);
        std::vector<ncclComm_t> comms(loc.size(), nullptr);
        G_NCCL(r->CommInitAll(comms.data(), (int)loc.size(), devs.data()));
        for (size_t k = 0; k < loc.size(); ++k) { loc[k].comm = comms[k]; loc[k].rank = (int)k; }
        return count_world((int)loc.size());
    }
    int init_comm_rank(const void* id128, int rank, int nranks)
    {
        Rccl* r = rccl();
        if (!r) return gfail(ISMPC_E_NO_DEVICE, "RCCL could not be loaded: " + g_rccl.err);
        static_assert(sizeof(ncclUniqueId) == ISMPC_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes");
        ncclUniqueId id; std::memcpy(&id, id128, sizeof id);
        DevGuard gd(loc[0].device); G_HIP(gd.err);
        G_NCCL(r->CommInitRank(&loc[0].comm, nranks, id, rank));
        loc[0].rank = rank;
        return count_world(nranks);
    }
    int count_world(int expected)
    {
        int c = 0;
        G_NCCL(g_rccl.CommCount(loc[0].comm, &c));
        if (c != expected) return gfail(ISMPC_E_NO_DEVICE, "RCCL reports " + std::to_string(c) + " ranks, expected " + std::to_string(expected));
        world = c;
        return ISMPC_OK;
    }
    int sync()
    {
        for (Local& l : loc) {
            DevGuard gd(l.device); G_HIP(gd.err);
            G_HIP(hipStreamSynchronize(l.launch)); G_HIP(hipStreamSynchronize(l.side));
        }
        return ISMPC_OK;
    }
    int reserve_all(int batch)
    {
        for (Local& l : loc) {
            if (batch <= l.all_cap) continue;
            DevGuard gd(l.device); G_HIP(gd.err);
            G_HIP(hipStreamSynchronize(l.launch)); G_HIP(hipStreamSynchronize(l.side));
            for (int b = 0; b < 2; ++b) {
                if (l.d_all[b]) G_HIP(hipFree(l.d_all[b]));
                l.d_all[b] = nullptr;
                G_HIP(hipMalloc((void**)&l.d_all[b], rec * (size_t)batch));
                l.gathered_set[b] = false;
            }
            l.all_cap = batch;
        }
        return ISMPC_OK;
    }
    int reserve_in(Local& l, int slot, size_t bytes)
    {
        if (bytes <= l.in_cap[slot]) return ISMPC_OK;
        G_HIP(hipStreamSynchronize(l.launch));
        if (l.d_in[slot]) G_HIP(hipFree(l.d_in[slot]));
        l.d_in[slot] = nullptr; l.in_cap[slot] = 0;
        G_HIP(hipMalloc(&l.d_in[slot], bytes));
        l.in_cap[slot] = bytes;
        return ISMPC_OK;
    }
    // before the kernel of a step writes buffer b: the collective that last read it is done (stream-side)
    int before_launch(Local& l, int b)
    {
        if (l.gathered_set[b]) G_HIP(hipStreamWaitEvent(l.launch, l.gathered[b], 0));
        return ISMPC_OK;
    }
    // the tick-major staging of a rollout's trajectory: grows only after this device's launch and side streams have drained
    int reserve_stage(Local& l, size_t bytes)
    {
        if (bytes <= l.stage_cap) return ISMPC_OK;
        G_HIP(hipStreamSynchronize(l.launch)); G_HIP(hipStreamSynchronize(l.side));
        if (l.d_stage) G_HIP(hipFree(l.d_stage));
        l.d_stage = nullptr; l.stage_cap = 0;
        G_HIP(hipMalloc(&l.d_stage, bytes));
        l.stage_cap = bytes;
        return ISMPC_OK;
    }
    // after every local kernel of the step is enqueued: the one collective, on the side streams.  Event slot b; every part is gathered
    // in place inside the same ncclGroupStart / ncclGroupEnd (no part: the events alone, no RCCL call).
    int gather(int batch, int b, const Part* parts, int n_parts)
    {
        for (Local& l : loc) {
            DevGuard gd(l.device); G_HIP(gd.err);
            G_HIP(hipEventRecord(l.computed[b], l.launch));
            G_HIP(hipStreamWaitEvent(l.side, l.computed[b], 0));
        }
        Rccl& r = g_rccl;
        // (ISMPC_GROUP_FORCE_RAGGED=1: the all-gather-v form for every batch -- how a one-GPU box tests it)
        static const bool force_ragged = std::getenv("ISMPC_GROUP_FORCE_RAGGED") != nullptr;
        const bool equal = batch % world == 0 && !force_ragged;
        if (n_parts > 0) G_NCCL(r.GroupStart());
        for (int q = 0; q < n_parts; ++q) for (size_t k = 0; k < loc.size(); ++k) {
            Local& l = loc[k];
            unsigned char* all = parts[q].base[k]; const size_t rec = parts[q].bytes;
            int first, count; shard(batch, l.rank, world, &first, &count);
            if (equal) {
                // in place: this rank's block already sits at recvbuff + rank * sendcount
                ncclResult_t e = r.AllGather(all + rec * (size_t)first, all, rec * (size_t)count, ncclUint8, l.comm, l.side);
                if (e != ncclSuccess) { (void)r.GroupEnd(); return gfail(ISMPC_E_NO_DEVICE, std::string("ncclAllGather: ") + r.GetErrorString(e)); }
            } else {
                // ragged shards: all-gather-v as one fused group of in-place broadcasts, root = owner of the block
                for (int root = 0; root < world; ++root) {
                    int f2, c2; shard(batch, root, world, &f2, &c2);
                    if (c2 == 0) continue;
                    unsigned char* blk = all + rec * (size_t)f2;
                    ncclResult_t e = r.Broadcast(blk, blk, rec * (size_t)c2, ncclUint8, root, l.comm, l.side);
                    if (e != ncclSuccess) { (void)r.GroupEnd(); return gfail(ISMPC_E_NO_DEVICE, std::string("ncclBroadcast: ") + r.GetErrorString(e)); }
                }
            }
        }
        if (n_parts > 0) G_NCCL(r.GroupEnd());
        for (Local& l : loc) {
            DevGuard gd(l.device); G_HIP(gd.err);
            G_HIP(hipEventRecord(l.gathered[b], l.side));
            l.gathered_set[b] = true;
        }
        return ISMPC_OK;
    }
    // the gathered output records of a tick step: buffer b of every local device
    int gather_step(int batch, int b)
    {
        Part p; p.bytes = rec;
        for (Local& l : loc) p.base.push_back(l.d_all[b]);
        return gather(batch, b, &p, 1);
    }
    int wait_on(int k, int b, void* stream)
    {
        if (k < 0 || k >= (int)loc.size()) return gfail(ISMPC_E_INVALID, "bad argument");
        Local& l = loc[k];
        DevGuard gd(l.device); G_HIP(gd.err);
        if (l.gathered_set[b]) G_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), l.gathered[b], 0));
        return ISMPC_OK;
    }
    // What the rollout entry points refuse before the device is touched (the single-device calls' own list, and the pointer lists).
    int check_rollout(int batch, const void* const* state, int ticks, const void* const* pushes, int n_push, int stride,
                      void* const* traj_all, void* const* summary_all) const
    {
        if (batch < 0) return gfail(ISMPC_E_INVALID, "negative batch");
        if (ticks < 0) return gfail(ISMPC_E_INVALID, "negative ticks");
        if (stride < 1) return gfail(ISMPC_E_INVALID, "traj_stride < 1");
        if (n_push < 0) return gfail(ISMPC_E_INVALID, "negative n_push");
        if (n_push > 0 && !pushes) return gfail(ISMPC_E_INVALID, "n_push > 0 with a null push table list");
        if (batch > 0 && !state) return gfail(ISMPC_E_INVALID, "null state list");
        for (size_t k = 0; batch > 0 && k < loc.size(); ++k) {
            int first, count; shard(batch, loc[k].rank, world, &first, &count);
            const std::string dev = " of local device " + std::to_string(k);
            if (count > 0 && !state[k]) return gfail(ISMPC_E_INVALID, "null state shard" + dev);
            if (count > 0 && n_push > 0 && !pushes[k]) return gfail(ISMPC_E_INVALID, "null push table" + dev);
            if (summary_all && !summary_all[k]) return gfail(ISMPC_E_INVALID, "null summary buffer" + dev);
            if (traj_all && !traj_all[k]) return gfail(ISMPC_E_INVALID, "null trajectory buffer" + dev);
            if (traj_all && (reinterpret_cast<uintptr_t>(traj_all[k]) & 15)) return gfail(ISMPC_E_INVALID, "trajectory buffer" + dev + " is not 16-byte aligned");
        }
        return ISMPC_OK;
    }
    // The rollout of both formulations, arguments checked.  run(k, count, traj, summary, stream) enqueues the single-device closed loop
    // of local device k's shard: `traj` tick-major (the staging buffer) or NULL, `summary` at its final position or NULL.
    template <class Run>
    int rollout(int batch, int rows, void* const* traj_all, void* const* summary_all, size_t summary_bytes, Run run)
    {
        const bool want_traj = traj_all && rows > 0;
        for (size_t k = 0; k < loc.size(); ++k) {
            Local& l = loc[k];
            int first, count; shard(batch, l.rank, world, &first, &count);
            DevGuard gd(l.device); G_HIP(gd.err);
            int rc = want_traj ? reserve_stage(l, rec * (size_t)rows * (size_t)count) : ISMPC_OK;
            if (rc == ISMPC_OK) rc = before_launch(l, ROLL);      // the previous rollout's collective may still read or write the caller's buffers
            if (rc != ISMPC_OK) return rc;
            if (count == 0) continue;                              // nothing to launch; the rank still takes part in the collective
            unsigned char* summary = summary_all ? static_cast<unsigned char*>(summary_all[k]) + summary_bytes * (size_t)first : nullptr;
            rc = run((int)k, count, want_traj ? l.d_stage : nullptr, summary, l.launch);
            if (rc == ISMPC_OK && want_traj)
                rc = pack_records(l.d_stage, rows, count, static_cast<unsigned char*>(traj_all[k]) + rec * (size_t)first * (size_t)rows, l.launch);
            if (rc != ISMPC_OK) return rc;
        }
        Part parts[2]; int n = 0;
        if (summary_all) { parts[n].bytes = summary_bytes; for (size_t k = 0; k < loc.size(); ++k) parts[n].base.push_back(static_cast<unsigned char*>(summary_all[k])); ++n; }
        if (want_traj) { parts[n].bytes = rec * (size_t)rows; for (size_t k = 0; k < loc.size(); ++k) parts[n].base.push_back(static_cast<unsigned char*>(traj_all[k])); ++n; }
        return gather(batch, ROLL, parts, n);
    }
    int reserve_rollout(int max_batch, int max_rows)
    {
        for (Local& l : loc) {
            int first, count; shard(max_batch, l.rank, world, &first, &count);
            DevGuard gd(l.device); G_HIP(gd.err);
            const int rc = reserve_stage(l, rec * (size_t)max_rows * (size_t)count);
            if (rc != ISMPC_OK) return rc;
        }
        return ISMPC_OK;
    }
    // the launch stream of local device k will not start later work before everything enqueued so far on `stream` is done
    int order_after(int k, void* stream)
    {
        if (k < 0 || k >= (int)loc.size()) return gfail(ISMPC_E_INVALID, "bad argument");
        Local& l = loc[k];
        DevGuard gd(l.device); G_HIP(gd.err);
        G_HIP(hipEventRecord(l.after, static_cast<hipStream_t>(stream)));
        G_HIP(hipStreamWaitEvent(l.launch, l.after, 0));
        return ISMPC_OK;
    }
    void destroy()
    {
        for (Local& l : loc) {
            DevGuard gd(l.device);
            if (l.launch) (void)hipStreamSynchronize(l.launch);
            if (l.side) (void)hipStreamSynchronize(l.side);
            if (l.comm && g_rccl.lib) (void)g_rccl.CommDestroy(l.comm);
            for (int b = 0; b < 2; ++b) if (l.d_all[b]) (void)hipFree(l.d_all[b]);
            for (int b = 0; b < 3; ++b) {
                if (l.computed[b]) (void)hipEventDestroy(l.computed[b]);
                if (l.gathered[b]) (void)hipEventDestroy(l.gathered[b]);
            }
            if (l.d_stage) (void)hipFree(l.d_stage);
            for (int k = 0; k < 4; ++k) if (l.d_in[k]) (void)hipFree(l.d_in[k]);
            if (l.after) (void)hipEventDestroy(l.after);
            if (l.launch) (void)hipStreamDestroy(l.launch);
            if (l.side) (void)hipStreamDestroy(l.side);
        }
        loc.clear();
    }
};

int check_devices(const int* devices, int n)
{
    if (!devices || n < 1) return gfail(ISMPC_E_INVALID, "a group needs at least one device");
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have < 1) { (void)hipGetLastError(); return gfail(ISMPC_E_NO_DEVICE, "no HIP device: the ISMPC hot path has no CPU fallback"); }
    for (int k = 0; k < n; ++k) {
        if (devices[k] < 0 || devices[k] >= have) return gfail(ISMPC_E_INVALID, "device ordinal " + std::to_string(devices[k]) + " outside [0, " + std::to_string(have) + ")");
        for (int j = 0; j < k; ++j) if (devices[j] == devices[k] && !(rccl() && g_rccl.test_double))
            return gfail(ISMPC_E_INVALID, "a device appears twice in the group (RCCL needs one rank per GPU)");
    }
    return ISMPC_OK;
}

}  // namespace

struct ismpc_group   { Core core; std::vector<ismpc_handle*> h; };
struct ismpc_a_group { Core core; std::vector<ismpc_a_handle*> h; };

extern "C" {

const char* ismpc_group_last_error(void) { return g_gerr.c_str(); }

int ismpc_group_rccl_version(void)
{
    Rccl* r = rccl(); int v = 0;
    if (!r || r->GetVersion(&v) != ncclSuccess) return 0;
    return v;
}

int ismpc_shard_range(int batch, int rank, int world, int* first, int* count)
{
    if (batch < 0 || world < 1 || rank < 0 || rank >= world || !first || !count) return gfail(ISMPC_E_INVALID, "bad argument");
    shard(batch, rank, world, first, count);
    return ISMPC_OK;
}

int ismpc_group_unique_id(void* id128)
{
    if (!id128) return gfail(ISMPC_E_INVALID, "null argument");
    Rccl* r = rccl();
    if (!r) return gfail(ISMPC_E_NO_DEVICE, "RCCL could not be loaded: " + g_rccl.err);
    ncclUniqueId id;
    G_NCCL(r->GetUniqueId(&id));
    std::memcpy(id128, &id, sizeof id);
    return ISMPC_OK;
}

// ======================================================================================================================
// Formulation B
// ======================================================================================================================
static int b_build(ismpc_group* g, const ismpc_params* params, const double* ftsp, int rows)
{
    for (Local& l : g->core.loc) {
        ismpc_handle* h = nullptr;
        const int rc = ismpc_create(params, ftsp, rows, l.device, &h);
        if (rc != ISMPC_OK) return gfail(rc, std::string("ismpc_create on device ") + std::to_string(l.device) + ": " + ismpc_last_error());
        g->h.push_back(h);
    }
    return g->core.init_streams();
}

void ismpc_group_destroy(ismpc_group* g)
{
    if (!g) return;
    g->core.destroy();
    for (ismpc_handle* h : g->h) ismpc_destroy(h);
    delete g;
}

int ismpc_group_create(const ismpc_params* params, const double* ftsp, int rows, const int* devices, int n, ismpc_group** out)
{
    if (!out) return gfail(ISMPC_E_INVALID, "null argument");
    *out = nullptr;
    int rc = check_devices(devices, n);
    if (rc != ISMPC_OK) return rc;
    ismpc_group* g = new ismpc_group();
    g->core.loc.resize(n);
    for (int k = 0; k < n; ++k) g->core.loc[k].device = devices[k];
    rc = b_build(g, params, ftsp, rows);
    if (rc == ISMPC_OK) rc = g->core.init_comm_all();
    if (rc != ISMPC_OK) { const std::string keep = g_gerr; ismpc_group_destroy(g); g_gerr = keep; return rc; }
    *out = g;
    return ISMPC_OK;
}

int ismpc_group_create_rank(const ismpc_params* params, const double* ftsp, int rows, int device, const void* id128, int rank, int world, ismpc_group** out)
{
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return gfail(ISMPC_E_INVALID, "bad argument");
    *out = nullptr;
    int rc = check_devices(&device, 1);
    if (rc != ISMPC_OK) return rc;
    ismpc_group* g = new ismpc_group();
    g->core.loc.resize(1);
    g->core.loc[0].device = device;
    rc = b_build(g, params, ftsp, rows);
    if (rc == ISMPC_OK) rc = g->core.init_comm_rank(id128, rank, world);
    if (rc != ISMPC_OK) { const std::string keep = g_gerr; ismpc_group_destroy(g); g_gerr = keep; return rc; }
    *out = g;
    return ISMPC_OK;
}

int ismpc_group_world(const ismpc_group* g) { return g ? g->core.world : ISMPC_E_INVALID; }
int ismpc_group_local(const ismpc_group* g) { return g ? (int)g->core.loc.size() : ISMPC_E_INVALID; }
int ismpc_group_rank(const ismpc_group* g, int local) { return (g && local >= 0 && local < (int)g->core.loc.size()) ? g->core.loc[local].rank : ISMPC_E_INVALID; }
ismpc_handle* ismpc_group_handle(ismpc_group* g, int local) { return (g && local >= 0 && local < (int)g->h.size()) ? g->h[local] : nullptr; }
int ismpc_group_sync(ismpc_group* g) { return g ? g->core.sync() : gfail(ISMPC_E_INVALID, "null group"); }
int ismpc_group_order_after(ismpc_group* g, int local, void* stream) { return g ? g->core.order_after(local, stream) : gfail(ISMPC_E_INVALID, "null group"); }

int ismpc_group_reserve(ismpc_group* g, int max_batch)
{
    if (!g || max_batch < 0) return gfail(ISMPC_E_INVALID, "bad argument");
    int rc = g->core.reserve_all(max_batch);
    for (size_t k = 0; rc == ISMPC_OK && k < g->h.size(); ++k) {
        int first, count; shard(max_batch, g->core.loc[k].rank, g->core.world, &first, &count);
        rc = ismpc_reserve(g->h[k], count + 1);
        if (rc != ISMPC_OK) return gfail(rc, ismpc_last_error());
    }
    return rc;
}

int ismpc_group_step_device(ismpc_group* g, int batch, const ismpc_tick_in* const* in_dev, int buf)
{
    if (!g || batch < 0 || (buf != 0 && buf != 1) || (batch > 0 && !in_dev)) return gfail(ISMPC_E_INVALID, "bad argument");
    if (batch == 0) return ISMPC_OK;
    Core& c = g->core;
    int rc = c.reserve_all(batch);
    if (rc != ISMPC_OK) return rc;
    for (size_t k = 0; k < c.loc.size(); ++k) {
        Local& l = c.loc[k];
        int first, count; shard(batch, l.rank, c.world, &first, &count);
        DevGuard gd(l.device); G_HIP(gd.err);
        rc = c.before_launch(l, buf);
        if (rc != ISMPC_OK) return rc;
        if (count > 0) {
            if (!in_dev[k]) return gfail(ISMPC_E_INVALID, "null shard pointer");
            rc = ismpc_solve_batch_device(g->h[k], count, in_dev[k], reinterpret_cast<ismpc_tick_out*>(l.d_all[buf]) + first, nullptr, l.launch);
            if (rc != ISMPC_OK) return gfail(rc, ismpc_last_error());
        }
    }
    return c.gather_step(batch, buf);
}

int ismpc_group_result_device(ismpc_group* g, int local, int buf, ismpc_tick_out** out_dev)
{
    if (!g || !out_dev || local < 0 || local >= (int)g->core.loc.size() || (buf != 0 && buf != 1)) return gfail(ISMPC_E_INVALID, "bad argument");
    *out_dev = reinterpret_cast<ismpc_tick_out*>(g->core.loc[local].d_all[buf]);
    return ISMPC_OK;
}

int ismpc_group_wait_on(ismpc_group* g, int local, int buf, void* stream)
{
    if (!g || local < 0 || local >= (int)g->core.loc.size() || (buf != 0 && buf != 1)) return gfail(ISMPC_E_INVALID, "bad argument");
    Local& l = g->core.loc[local];
    DevGuard gd(l.device); G_HIP(gd.err);
    if (l.gathered_set[buf]) G_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), l.gathered[buf], 0));
    return ISMPC_OK;
}

int ismpc_records_to_instance_major_device(const void* tick_major, int rows, int count, void* dst_block, void* stream)
{
    return pack_records(tick_major, rows, count, dst_block, static_cast<hipStream_t>(stream));
}

int ismpc_group_rollout_mc_device(ismpc_group* g, int batch, ismpc_tick_in* const* state_dev, int first_frame, int ticks,
                                  const ismpc_push* const* pushes_dev, int n_push, int traj_stride,
                                  ismpc_tick_out* const* traj_all_dev, ismpc_rollout_summary* const* summary_all_dev)
{
    if (!g) return gfail(ISMPC_E_INVALID, "null group");
    if (first_frame < 0) return gfail(ISMPC_E_INVALID, "negative first_frame");
    void* const* traj = reinterpret_cast<void* const*>(traj_all_dev); void* const* summ = reinterpret_cast<void* const*>(summary_all_dev);
    const int rc = g->core.check_rollout(batch, reinterpret_cast<const void* const*>(state_dev), ticks, reinterpret_cast<const void* const*>(pushes_dev),
                                         n_push, traj_stride, traj, summ);
    if (rc != ISMPC_OK || batch == 0) return rc;
    return g->core.rollout(batch, ticks / traj_stride, traj, summ, sizeof(ismpc_rollout_summary),
        [&](int k, int count, void* stage, void* summary, hipStream_t s) {
            const int r = ismpc_rollout_mc_device(g->h[k], count, state_dev[k], first_frame, ticks, n_push > 0 ? pushes_dev[k] : nullptr, n_push, traj_stride,
                                                  static_cast<ismpc_tick_out*>(stage), static_cast<ismpc_rollout_summary*>(summary), s);
            return r == ISMPC_OK ? r : gfail(r, ismpc_last_error());
        });
}

int ismpc_group_rollout_wait_on(ismpc_group* g, int local, void* stream) { return g ? g->core.wait_on(local, ROLL, stream) : gfail(ISMPC_E_INVALID, "null group"); }

int ismpc_group_reserve_rollout(ismpc_group* g, int max_batch, int max_rows)
{
    if (!g || max_batch < 0 || max_rows < 0) return gfail(ISMPC_E_INVALID, "bad argument");
    int rc = g->core.reserve_rollout(max_batch, max_rows);
    for (size_t k = 0; rc == ISMPC_OK && k < g->h.size(); ++k) {
        int first, count; shard(max_batch, g->core.loc[k].rank, g->core.world, &first, &count);
        rc = ismpc_reserve(g->h[k], count + 1);
        if (rc != ISMPC_OK) return gfail(rc, ismpc_last_error());
    }
    return rc;
}

int ismpc_group_solve_batch(ismpc_group* g, int batch, const ismpc_tick_in* in_host, ismpc_tick_out* out_host)
{
    if (!g || batch < 0 || (batch > 0 && (!in_host || !out_host))) return gfail(ISMPC_E_INVALID, "bad argument");
    if (batch == 0) return ISMPC_OK;
    Core& c = g->core;
    int rc = c.reserve_all(batch);
    if (rc != ISMPC_OK) return rc;
    std::vector<const ismpc_tick_in*> shards(c.loc.size(), nullptr);
    for (size_t k = 0; k < c.loc.size(); ++k) {
        Local& l = c.loc[k];
        int first, count; shard(batch, l.rank, c.world, &first, &count);
        DevGuard gd(l.device); G_HIP(gd.err);
        rc = c.reserve_in(l, 0, sizeof(ismpc_tick_in) * (size_t)(count > 0 ? count : 1));
        if (rc != ISMPC_OK) return rc;
        if (count > 0) G_HIP(hipMemcpyAsync(l.d_in[0], in_host + first, sizeof(ismpc_tick_in) * (size_t)count, hipMemcpyHostToDevice, l.launch));
        shards[k] = static_cast<const ismpc_tick_in*>(l.d_in[0]);
    }
    rc = ismpc_group_step_device(g, batch, shards.data(), 0);
    if (rc != ISMPC_OK) return rc;
    {   // every device holds all records now; the caller's copy comes from the first local one
        Local& l = c.loc[0];
        DevGuard gd(l.device); G_HIP(gd.err);
        G_HIP(hipMemcpyAsync(out_host, l.d_all[0], sizeof(ismpc_tick_out) * (size_t)batch, hipMemcpyDeviceToHost, l.side));
    }
    return c.sync();
}

// ======================================================================================================================
// Formulation A
// ======================================================================================================================
static int a_build(ismpc_a_group* g, const ismpc_a_params* p, const double* center)
{
    for (Local& l : g->core.loc) {
        ismpc_a_handle* h = nullptr;
        const int rc = ismpc_a_create(p, center, l.device, &h);
        if (rc != ISMPC_OK) return gfail(rc, std::string("ismpc_a_create on device ") + std::to_string(l.device) + ": " + ismpc_a_last_error());
        g->h.push_back(h);
    }
    return g->core.init_streams();
}

void ismpc_a_group_destroy(ismpc_a_group* g)
{
    if (!g) return;
    g->core.destroy();
    for (ismpc_a_handle* h : g->h) ismpc_a_destroy(h);
    delete g;
}

int ismpc_a_group_create(const ismpc_a_params* p, const double* center, const int* devices, int n, ismpc_a_group** out)
{
    if (!out) return gfail(ISMPC_E_INVALID, "null argument");
    *out = nullptr;
    int rc = check_devices(devices, n);
    if (rc != ISMPC_OK) return rc;
    ismpc_a_group* g = new ismpc_a_group();
    g->core.loc.resize(n);
    for (int k = 0; k < n; ++k) g->core.loc[k].device = devices[k];
    rc = a_build(g, p, center);
    if (rc == ISMPC_OK) rc = g->core.init_comm_all();
    if (rc != ISMPC_OK) { const std::string keep = g_gerr; ismpc_a_group_destroy(g); g_gerr = keep; return rc; }
    *out = g;
    return ISMPC_OK;
}

int ismpc_a_group_create_rank(const ismpc_a_params* p, const double* center, int device, const void* id128, int rank, int world, ismpc_a_group** out)
{
    if (!out || !id128 || world < 1 || rank < 0 || rank >= world) return gfail(ISMPC_E_INVALID, "bad argument");
    *out = nullptr;
    int rc = check_devices(&device, 1);
    if (rc != ISMPC_OK) return rc;
    ismpc_a_group* g = new ismpc_a_group();
    g->core.loc.resize(1);
    g->core.loc[0].device = device;
    rc = a_build(g, p, center);
    if (rc == ISMPC_OK) rc = g->core.init_comm_rank(id128, rank, world);
    if (rc != ISMPC_OK) { const std::string keep = g_gerr; ismpc_a_group_destroy(g); g_gerr = keep; return rc; }
    *out = g;
    return ISMPC_OK;
}

int ismpc_a_group_world(const ismpc_a_group* g) { return g ? g->core.world : ISMPC_E_INVALID; }
int ismpc_a_group_local(const ismpc_a_group* g) { return g ? (int)g->core.loc.size() : ISMPC_E_INVALID; }
int ismpc_a_group_rank(const ismpc_a_group* g, int local) { return (g && local >= 0 && local < (int)g->core.loc.size()) ? g->core.loc[local].rank : ISMPC_E_INVALID; }
ismpc_a_handle* ismpc_a_group_handle(ismpc_a_group* g, int local) { return (g && local >= 0 && local < (int)g->h.size()) ? g->h[local] : nullptr; }
int ismpc_a_group_sync(ismpc_a_group* g) { return g ? g->core.sync() : gfail(ISMPC_E_INVALID, "null group"); }
int ismpc_a_group_order_after(ismpc_a_group* g, int local, void* stream) { return g ? g->core.order_after(local, stream) : gfail(ISMPC_E_INVALID, "null group"); }

int ismpc_a_group_add_plan(ismpc_a_group* g, const double* center)
{
    if (!g || !center) return gfail(ISMPC_E_INVALID, "bad argument");
    int idx = -1;
    for (ismpc_a_handle* h : g->h) {
        const int r = ismpc_a_add_plan(h, center);
        if (r < 0) return gfail(r, ismpc_a_last_error());
        if (idx >= 0 && r != idx) return gfail(ISMPC_E_INVALID, "plan indices differ between devices");
        idx = r;
    }
    return idx;
}

int ismpc_a_group_set_precision(ismpc_a_group* g, int fp32)
{
    if (!g) return gfail(ISMPC_E_INVALID, "null group");
    for (ismpc_a_handle* h : g->h) {
        const int r = ismpc_a_set_precision(h, fp32);
        if (r != ISMPC_OK) return gfail(r, ismpc_a_last_error());
    }
    return ISMPC_OK;
}

int ismpc_a_group_reserve(ismpc_a_group* g, int max_batch)
{
    if (!g || max_batch < 0) return gfail(ISMPC_E_INVALID, "bad argument");
    int rc = g->core.reserve_all(max_batch);
    for (size_t k = 0; rc == ISMPC_OK && k < g->h.size(); ++k) {
        int first, count; shard(max_batch, g->core.loc[k].rank, g->core.world, &first, &count);
        rc = ismpc_a_reserve(g->h[k], count + 1);
        if (rc != ISMPC_OK) return gfail(rc, ismpc_a_last_error());
    }
    return rc;
}

int ismpc_a_group_step_device(ismpc_a_group* g, int batch, ismpc_a_state* const* state_dev, const ismpc_a_inst* const* inst_dev,
                              const double* const* push_dev, int buf)
{
    if (!g || batch < 0 || (buf != 0 && buf != 1) || (batch > 0 && !state_dev)) return gfail(ISMPC_E_INVALID, "bad argument");
    if (batch == 0) return ISMPC_OK;
    Core& c = g->core;
    int rc = c.reserve_all(batch);
    if (rc != ISMPC_OK) return rc;
    for (size_t k = 0; k < c.loc.size(); ++k) {
        Local& l = c.loc[k];
        int first, count; shard(batch, l.rank, c.world, &first, &count);
        DevGuard gd(l.device); G_HIP(gd.err);
        rc = c.before_launch(l, buf);
        if (rc != ISMPC_OK) return rc;
        if (count > 0) {
            if (!state_dev[k]) return gfail(ISMPC_E_INVALID, "null shard pointer");
            ismpc_a_out* dst = reinterpret_cast<ismpc_a_out*>(l.d_all[buf]) + first;
            const double* push = push_dev ? push_dev[k] : nullptr;
            const ismpc_a_inst* inst = inst_dev ? inst_dev[k] : nullptr;
            rc = inst ? ismpc_a_tick_batch_inst_device(g->h[k], count, state_dev[k], inst, push, dst, l.launch)
                      : ismpc_a_tick_batch_device(g->h[k], count, state_dev[k], push, dst, l.launch);
            if (rc != ISMPC_OK) return gfail(rc, ismpc_a_last_error());
        }
    }
    return c.gather_step(batch, buf);
}

int ismpc_a_group_result_device(ismpc_a_group* g, int local, int buf, ismpc_a_out** out_dev)
{
    if (!g || !out_dev || local < 0 || local >= (int)g->core.loc.size() || (buf != 0 && buf != 1)) return gfail(ISMPC_E_INVALID, "bad argument");
    *out_dev = reinterpret_cast<ismpc_a_out*>(g->core.loc[local].d_all[buf]);
    return ISMPC_OK;
}

int ismpc_a_group_wait_on(ismpc_a_group* g, int local, int buf, void* stream)
{
    if (!g || local < 0 || local >= (int)g->core.loc.size() || (buf != 0 && buf != 1)) return gfail(ISMPC_E_INVALID, "bad argument");
    Local& l = g->core.loc[local];
    DevGuard gd(l.device); G_HIP(gd.err);
    if (l.gathered_set[buf]) G_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(stream), l.gathered[buf], 0));
    return ISMPC_OK;
}

int ismpc_a_group_rollout_mc_device(ismpc_a_group* g, int batch, ismpc_a_state* const* state_dev, const ismpc_a_inst* const* inst_dev, int ticks,
                                    const ismpc_a_push* const* pushes_dev, int n_push, int traj_stride,
                                    ismpc_a_out* const* traj_all_dev, ismpc_a_rollout_summary* const* summary_all_dev)
{
    if (!g) return gfail(ISMPC_E_INVALID, "null group");
    void* const* traj = reinterpret_cast<void* const*>(traj_all_dev); void* const* summ = reinterpret_cast<void* const*>(summary_all_dev);
    const int rc = g->core.check_rollout(batch, reinterpret_cast<const void* const*>(state_dev), ticks, reinterpret_cast<const void* const*>(pushes_dev),
                                         n_push, traj_stride, traj, summ);
    if (rc != ISMPC_OK || batch == 0) return rc;
    return g->core.rollout(batch, ticks / traj_stride, traj, summ, sizeof(ismpc_a_rollout_summary),
        [&](int k, int count, void* stage, void* summary, hipStream_t s) {
            const int r = ismpc_a_rollout_mc_device(g->h[k], count, state_dev[k], inst_dev ? inst_dev[k] : nullptr, ticks, n_push > 0 ? pushes_dev[k] : nullptr, n_push,
                                                    traj_stride, static_cast<ismpc_a_out*>(stage), static_cast<ismpc_a_rollout_summary*>(summary), s);
            return r == ISMPC_OK ? r : gfail(r, ismpc_a_last_error());
        });
}

int ismpc_a_group_rollout_wait_on(ismpc_a_group* g, int local, void* stream) { return g ? g->core.wait_on(local, ROLL, stream) : gfail(ISMPC_E_INVALID, "null group"); }

int ismpc_a_group_reserve_rollout(ismpc_a_group* g, int max_batch, int max_rows)
{
    if (!g || max_batch < 0 || max_rows < 0) return gfail(ISMPC_E_INVALID, "bad argument");
    int rc = g->core.reserve_rollout(max_batch, max_rows);
    for (size_t k = 0; rc == ISMPC_OK && k < g->h.size(); ++k) {
        int first, count; shard(max_batch, g->core.loc[k].rank, g->core.world, &first, &count);
        rc = ismpc_a_reserve(g->h[k], count + 1);
        if (rc != ISMPC_OK) return gfail(rc, ismpc_a_last_error());
    }
    return rc;
}

int ismpc_a_group_tick_batch(ismpc_a_group* g, int batch, ismpc_a_state* state_host, const ismpc_a_inst* inst_host,
                             const double* push_host, ismpc_a_out* out_host)
{
    if (!g || batch < 0 || (batch > 0 && (!state_host || !out_host))) return gfail(ISMPC_E_INVALID, "bad argument");
    if (batch == 0) return ISMPC_OK;
    Core& c = g->core;
    int rc = c.reserve_all(batch);
    if (rc != ISMPC_OK) return rc;
    const size_t n = c.loc.size();
    std::vector<ismpc_a_state*> st(n, nullptr); std::vector<const ismpc_a_inst*> in(n, nullptr); std::vector<const double*> pu(n, nullptr);
    for (size_t k = 0; k < n; ++k) {
        Local& l = c.loc[k];
        int first, count; shard(batch, l.rank, c.world, &first, &count);
        const size_t cn = (size_t)(count > 0 ? count : 1);
        DevGuard gd(l.device); G_HIP(gd.err);
        rc = c.reserve_in(l, 0, sizeof(ismpc_a_state) * cn);
        if (rc == ISMPC_OK && inst_host) rc = c.reserve_in(l, 1, sizeof(ismpc_a_inst) * cn);
        if (rc == ISMPC_OK && push_host) rc = c.reserve_in(l, 2, 2 * sizeof(double) * cn);
        if (rc != ISMPC_OK) return rc;
        if (count > 0) {
            G_HIP(hipMemcpyAsync(l.d_in[0], state_host + first, sizeof(ismpc_a_state) * (size_t)count, hipMemcpyHostToDevice, l.launch));
            if (inst_host) G_HIP(hipMemcpyAsync(l.d_in[1], inst_host + first, sizeof(ismpc_a_inst) * (size_t)count, hipMemcpyHostToDevice, l.launch));
            if (push_host) G_HIP(hipMemcpyAsync(l.d_in[2], push_host + 2 * (size_t)first, 2 * sizeof(double) * (size_t)count, hipMemcpyHostToDevice, l.launch));
        }
        st[k] = static_cast<ismpc_a_state*>(l.d_in[0]);
        in[k] = inst_host ? static_cast<const ismpc_a_inst*>(l.d_in[1]) : nullptr;
        pu[k] = push_host ? static_cast<const double*>(l.d_in[2]) : nullptr;
    }
    rc = ismpc_a_group_step_device(g, batch, st.data(), in.data(), pu.data(), 0);
    if (rc != ISMPC_OK) return rc;
    for (size_t k = 0; k < n; ++k) {          // the advanced state of this process's shards goes back in place
        Local& l = c.loc[k];
        int first, count; shard(batch, l.rank, c.world, &first, &count);
        DevGuard gd(l.device); G_HIP(gd.err);
        if (count > 0) G_HIP(hipMemcpyAsync(state_host + first, l.d_in[0], sizeof(ismpc_a_state) * (size_t)count, hipMemcpyDeviceToHost, l.launch));
    }
    {
        Local& l = c.loc[0];
        DevGuard gd(l.device); G_HIP(gd.err);
        G_HIP(hipMemcpyAsync(out_host, l.d_all[0], sizeof(ismpc_a_out) * (size_t)batch, hipMemcpyDeviceToHost, l.side));
    }
    return c.sync();
}

}  // extern "C"
