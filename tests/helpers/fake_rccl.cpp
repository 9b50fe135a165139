// TEST DOUBLE, never part of the product: the eleven nccl* entry points csrc/ismpc_group.hip binds, implemented for several ranks
// inside ONE process and ONE host thread (the ncclCommInitAll shape: one process drives every GPU of the node) with device-to-device
// copies and events -- so that a group of 2, 3 or 8 ranks runs on the one GPU of a test box (tests/cpp/test_group_world.cpp) and a
// wrong offset, block or wait in the library shows as wrong bytes.  Built by tests/test_gpu_group.py (hipcc -shared -fPIC) and selected
// with ISMPC_RCCL_LIB in a process that maps no other RCCL.  ncclGetVersion reports 1: not "not loaded" (0), not a real RCCL (> 20000).
//
// A collective posted between ncclGroupStart and ncclGroupEnd is only recorded.  The outermost ncclGroupEnd matches the posts of the
// communicator's ranks by call order and, per collective,
//   (a) records a "ready" event on every participant's stream,
//   (b) on each destination stream waits for the sources' ready events, enqueues the copies and records a "done" event,
//   (c) makes every participant's stream wait for every other participant's done event
// -- (c) because a real collective completes on no rank before its peers hold that rank's data; it is what lets the library's
// gathered[b] event protect a block another rank still reads.  Every wait is enqueued after the record it waits for (a wait on an
// event never recorded is a no-op in HIP).  The all-gather is the general out-of-place one: recv + src_rank * bytes from the source's
// send, whatever the pointers are (a copy onto itself is skipped).  A group that ends with posts missing on some rank, or with ranks
// that disagree about a collective, returns ncclInvalidUsage and enqueues nothing: the double never waits for a post that does not come.
// Rank mode (ncclCommInitRank) exists for one rank only; more would need a blocking host thread per rank.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct Post { int kind; const void* send; void* recv; size_t bytes; int root; hipStream_t stream; };   // kind 0 = all-gather, 1 = broadcast
struct World { std::vector<ncclComm*> comms; int alive = 0; };

}  // namespace

struct ncclComm {
    World* world = nullptr; int rank = 0, device = 0;
    hipEvent_t ready = nullptr, done = nullptr;         // re-recorded per collective: a wait holds the record that preceded it
    std::vector<Post> posts;
};

namespace {

int g_depth = 0;                       // one host thread drives every rank: plain globals
std::vector<World*> g_touched;         // communicators with posts in the open group

struct OnDevice {
    int prev = -1; bool ok = true;
    explicit OnDevice(int d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != d) ok = hipSetDevice(d) == hipSuccess; }
    ~OnDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

size_t type_bytes(ncclDataType_t t)
{
    switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
    }
}

ncclComm* new_comm(World* w, int rank, int device)
{
    ncclComm* c = new ncclComm();
    c->world = w; c->rank = rank; c->device = device;
    OnDevice on(device);
    if (!on.ok || hipEventCreateWithFlags(&c->ready, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->done, hipEventDisableTiming) != hipSuccess) {
        if (c->ready) (void)hipEventDestroy(c->ready);
        delete c; return nullptr;
    }
    w->comms.push_back(c); ++w->alive;
    return c;
}

ncclResult_t post(ncclComm* c, const Post& p)
{
    if (!c || !c->world || (p.bytes && (!p.send || !p.recv))) return ncclInvalidArgument;
    const bool implicit = g_depth == 0;           // a collective outside a group is a group of its own
    if (implicit) ++g_depth;
    c->posts.push_back(p);
    if (std::find(g_touched.begin(), g_touched.end(), c->world) == g_touched.end()) g_touched.push_back(c->world);
    return implicit ? ncclGroupEnd() : ncclSuccess;
}

// every rank posted the same number of collectives, and the ranks agree about each one
bool matched(const World& w)
{
    const size_t n = w.comms[0]->posts.size();
    for (const ncclComm* c : w.comms) if (c->posts.size() != n) return false;
    for (size_t i = 0; i < n; ++i) {
        const Post& p0 = w.comms[0]->posts[i];
        if (p0.kind == 1 && (p0.root < 0 || p0.root >= (int)w.comms.size())) return false;
        for (const ncclComm* c : w.comms) { const Post& p = c->posts[i]; if (p.kind != p0.kind || p.bytes != p0.bytes || p.root != p0.root) return false; }
    }
    return true;
}

#define FK_HIP(expr) do { if ((expr) != hipSuccess) return ncclUnhandledCudaError; } while (0)

ncclResult_t run(World& w, size_t i)
{
    const int n = (int)w.comms.size();
    for (ncclComm* c : w.comms) {                                                        // (a)
        OnDevice on(c->device); if (!on.ok) return ncclUnhandledCudaError;
        FK_HIP(hipEventRecord(c->ready, c->posts[i].stream));
    }
    for (ncclComm* c : w.comms) {                                                        // (b)
        const Post& p = c->posts[i];
        OnDevice on(c->device); if (!on.ok) return ncclUnhandledCudaError;
        if (p.kind == 0) {
            for (int s = 0; s < n; ++s) if (s != c->rank) FK_HIP(hipStreamWaitEvent(p.stream, w.comms[s]->ready, 0));
            for (int s = 0; s < n; ++s) {
                unsigned char* dst = static_cast<unsigned char*>(p.recv) + (size_t)s * p.bytes;
                const void* src = w.comms[s]->posts[i].send;
                if (p.bytes && dst != src) FK_HIP(hipMemcpyAsync(dst, src, p.bytes, hipMemcpyDeviceToDevice, p.stream));
            }
        } else {
            if (p.root != c->rank) FK_HIP(hipStreamWaitEvent(p.stream, w.comms[p.root]->ready, 0));
            const void* src = w.comms[p.root]->posts[i].send;
            if (p.bytes && p.recv != src) FK_HIP(hipMemcpyAsync(p.recv, src, p.bytes, hipMemcpyDeviceToDevice, p.stream));
        }
        FK_HIP(hipEventRecord(c->done, p.stream));
    }
    for (ncclComm* c : w.comms) {                                                        // (c)
        OnDevice on(c->device); if (!on.ok) return ncclUnhandledCudaError;
        for (ncclComm* o : w.comms) if (o != c) FK_HIP(hipStreamWaitEvent(c->posts[i].stream, o->done, 0));
    }
    return ncclSuccess;
}

}  // namespace

extern "C" {

int ismpc_test_rccl_double = 1;        // the marker csrc/ismpc_group.hip looks for before it lets a device appear twice

ncclResult_t ncclGetVersion(int* version) { if (!version) return ncclInvalidArgument; *version = 1; return ncclSuccess; }

const char* ncclGetErrorString(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error (test double)";
    case ncclUnhandledCudaError: return "unhandled HIP error (test double)";
    case ncclInvalidArgument: return "invalid argument (test double)";
    case ncclInvalidUsage: return "invalid usage (test double)";
    default: return "error (test double)";
    }
}

ncclResult_t ncclGetUniqueId(ncclUniqueId* id)
{
    if (!id) return ncclInvalidArgument;
    std::memset(id->internal, 0, sizeof id->internal);
    std::strcpy(id->internal, "ismpc test double");
    return ncclSuccess;
}

ncclResult_t ncclCommInitAll(ncclComm_t* comms, int ndev, const int* devlist)
{
    if (!comms || ndev < 1) return ncclInvalidArgument;
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess) return ncclUnhandledCudaError;
    for (int k = 0; k < ndev; ++k) { const int d = devlist ? devlist[k] : k; if (d < 0 || d >= have) return ncclInvalidArgument; }   // repeated ordinals are fine here
    World* w = new World();
    for (int k = 0; k < ndev; ++k) {
        comms[k] = new_comm(w, k, devlist ? devlist[k] : k);
        if (!comms[k]) { for (int j = 0; j < k; ++j) { (void)ncclCommDestroy(comms[j]); comms[j] = nullptr; } if (k == 0) delete w; return ncclUnhandledCudaError; }
    }
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId, int rank)
{
    if (!comm) return ncclInvalidArgument;
    if (nranks != 1 || rank != 0) return ncclInvalidUsage;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return ncclUnhandledCudaError;
    World* w = new World();
    *comm = new_comm(w, 0, dev);
    if (!*comm) { delete w; return ncclUnhandledCudaError; }
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t c)
{
    if (!c) return ncclInvalidArgument;
    World* w = c->world;
    {
        OnDevice on(c->device);
        (void)hipEventDestroy(c->ready); (void)hipEventDestroy(c->done);
    }
    g_touched.erase(std::remove(g_touched.begin(), g_touched.end(), w), g_touched.end());
    for (ncclComm*& m : w->comms) if (m == c) m = nullptr;
    delete c;
    if (--w->alive == 0) delete w;
    return ncclSuccess;
}

ncclResult_t ncclCommCount(const ncclComm_t c, int* count)
{
    if (!c || !count) return ncclInvalidArgument;
    *count = (int)c->world->comms.size();
    return ncclSuccess;
}

ncclResult_t ncclGroupStart() { ++g_depth; return ncclSuccess; }

ncclResult_t ncclGroupEnd()
{
    if (g_depth < 1) return ncclInvalidUsage;
    if (--g_depth > 0) return ncclSuccess;
    std::vector<World*> worlds; worlds.swap(g_touched);
    ncclResult_t res = ncclSuccess;
    for (World* w : worlds) {
        bool whole = true; for (const ncclComm* c : w->comms) whole = whole && c != nullptr;
        if (!whole || !matched(*w)) res = ncclInvalidUsage;                              // validated for every communicator before anything is enqueued
    }
    for (World* w : worlds) {
        const size_t n = (w->comms.empty() || !w->comms[0]) ? 0 : w->comms[0]->posts.size();
        for (size_t i = 0; res == ncclSuccess && i < n; ++i) res = run(*w, i);
        for (ncclComm* c : w->comms) if (c) c->posts.clear();
    }
    return res;
}

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream)
{
    const size_t tb = type_bytes(datatype);
    if (!tb) return ncclInvalidArgument;
    return post(comm, Post{0, sendbuff, recvbuff, sendcount * tb, -1, stream});
}

ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm, hipStream_t stream)
{
    const size_t tb = type_bytes(datatype);
    if (!tb) return ncclInvalidArgument;
    return post(comm, Post{1, sendbuff, recvbuff, count * tb, root, stream});
}

}  // extern "C"
