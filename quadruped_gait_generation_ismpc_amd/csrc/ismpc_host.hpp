// Host plumbing shared by the three C ABIs (ismpc_hip.hip, ismpc_a_hip.hip, ismpc_group.hip): the device guard, the early return on a
// HIP error, and growth (stream-ordered or synchronous) of scratch that outlives a call.  Each ABI keeps its own thread-local error string and
// its own `int fail(code, message)`; the macros below take that function by name.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

namespace ismpc_host {
namespace {      // (internal linkage: each ABI's unit gets its own copy, the library exports none of this)

// Entry points run on the handle's device and leave the caller's current device as they found it (a torch process that
// drives several GPUs keeps allocating where it was).
struct DeviceGuard {
    int prev = -1, dev; hipError_t err = hipSuccess;
    explicit DeviceGuard(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};

constexpr int E_HIP = -2;      // what every ABI returns on a HIP error (ISMPC_E_NO_DEVICE)

// A handle H carries `hipStream_t last_stream; bool used;`: the stream of its previous launch.  Scratch that outlives the call
// that allocated it is used by later calls on whatever stream those pass: before it is re-allocated on stream `s`, the previous
// launch's stream -- if it is another one -- is drained, so the free cannot overtake kernels that still use the block.
template <class H> hipError_t grow_sync(H* h, hipStream_t s)
{
    if (h->used && h->last_stream != s) return hipStreamSynchronize(h->last_stream);
    return hipSuccess;
}
// Declared at the top of a launching call: remembers the stream of this launch when the call returns, however it returns.
template <class H> struct StreamMark { H* h; hipStream_t s; ~StreamMark() { h->last_stream = s; h->used = true; } };

}  // namespace
}  // namespace ismpc_host

// `fail_` is the including unit's own int fail(int code, const std::string& message), which records the message in that ABI's error string
#define ISMPC_HIP_TRY(fail_, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail_(ismpc_host::E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define ISMPC_ON_DEVICE(fail_, h_) ismpc_host::DeviceGuard guard_((h_)->device); ISMPC_HIP_TRY(fail_, guard_.err)
// Stream-ordered growth of such scratch: pointer `p_` of handle `h_` to `bytes_`, capacity `cap_` to `new_cap_` (no device-wide
// synchronisation inside an asynchronous entry point; callers that capture graphs size it beforehand with the ABI's reserve call).
// The pointer and the capacity never name a freed block: they are cleared before the allocation and the capacity is set only after
// it succeeded.  A macro so that a failing step returns from the entry point with its own text ("hipFreeAsync(h->zmark, s): ...").
#define ISMPC_GROW_ASYNC(fail_, h_, p_, cap_, new_cap_, bytes_, s_) do { \
    ISMPC_HIP_TRY(fail_, grow_sync(h_, s_)); \
    if (p_) ISMPC_HIP_TRY(fail_, hipFreeAsync(p_, s_)); \
    p_ = nullptr; cap_ = 0; \
    ISMPC_HIP_TRY(fail_, hipMallocAsync((void**)&p_, bytes_, s_)); \
    cap_ = new_cap_; } while (0)
// The synchronous twin, for set-up calls (the ABI's reserve): same order, same reason to be a macro ("hipFree(h->prev): ...").
#define ISMPC_GROW_SYNC(fail_, p_, cap_, new_cap_, bytes_) do { \
    if (p_) ISMPC_HIP_TRY(fail_, hipFree(p_)); \
    p_ = nullptr; cap_ = 0; \
    ISMPC_HIP_TRY(fail_, hipMalloc((void**)&p_, bytes_)); \
    cap_ = new_cap_; } while (0)
