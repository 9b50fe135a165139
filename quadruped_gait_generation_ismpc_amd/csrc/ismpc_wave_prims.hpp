// Wavefront (64 lanes) primitives shared by the Formulation B kernels (ismpc_hip.hip and its ismpc_b_*.hpp parts) and the
// Formulation A kernels (ismpc_a_hip.hip, ismpc_a_wave.hpp): DPP moves and scans, no LDS crossbar (ds_bpermute) on the critical path.
// DPP controls (GFX9 / CDNA): row_shl:n = 0x100+n, row_shr:n = 0x110+n, wave_shl:1 = 0x130,
// row_bcast:15 = 0x142, row_bcast:31 = 0x143.  A "row" is 16 lanes.
// Everything here is __forceinline__ and sets no floating-point pragma: the including unit's contraction setting holds.
#pragma once
#include <hip/hip_runtime.h>

namespace ismpc_wave {

template <int CTRL, int ROW_MASK, bool BOUND_ZERO>
__device__ __forceinline__ double dppv(double old, double src)
{
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, ROW_MASK, 0xf, BOUND_ZERO);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, ROW_MASK, 0xf, BOUND_ZERO);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK, bool BOUND_ZERO>
__device__ __forceinline__ float dppv(float old, float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, ROW_MASK, 0xf, BOUND_ZERO));
}
template <int LANE>
__device__ __forceinline__ double readlane64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), LANE), __builtin_amdgcn_readlane(__double2loint(v), LANE));
}
// inclusive prefix sum over lanes 0..lane
template <typename R> __device__ __forceinline__ R wave_scan_up(R v)
{
    v += dppv<0x111, 0xf, true>(R(0), v);
    v += dppv<0x112, 0xf, true>(R(0), v);
    v += dppv<0x114, 0xf, true>(R(0), v);
    v += dppv<0x118, 0xf, true>(R(0), v);
    v += dppv<0x142, 0xa, false>(R(0), v);      // rows 1,3 += lane 15 of the row below
    v += dppv<0x143, 0xc, false>(R(0), v);      // rows 2,3 += lane 31
    return v;
}
// wave-uniform sum of all 64 lanes
__device__ __forceinline__ double wave_sum(double v) { return readlane64<63>(wave_scan_up(v)); }
// sum over lanes strictly below this one
__device__ __forceinline__ double wave_prefix_excl(double v) { return wave_scan_up(v) - v; }
__device__ __forceinline__ double bcast0(double v) { return readlane64<0>(v); }

}  // namespace ismpc_wave
