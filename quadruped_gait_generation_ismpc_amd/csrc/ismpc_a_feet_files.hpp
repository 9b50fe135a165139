// Formulation A, what follows a batch's swing-foot rollout on the device:
//   ismpc_a_feet_summary_kernel       per instance, how far its foot plan block ended from the base plan (ismpc_a_feet_summary)
//   ismpc_a_foot_trajectories_kernel  the four foot files of every instance, bit for bit the host writer ismpc_a_foot_trajectories
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ismpc_a_feet.hpp"

namespace {

// ---- ismpc_a_feet_summary: one wavefront per instance, four per workgroup.  The block of an instance is rows x 8 contiguous doubles
// (about 7 KB): lane l reads doubles l, l + 64, ... of it and of the base plan, so every load of the wavefront is 512 contiguous bytes,
// and -- 64 being a multiple of 8 -- a lane stays on one column (l % 8) while a pass covers the 8 rows 8 p .. 8 p + 7, row l / 8 of them
// on lanes 8 (l / 8) .. 8 (l / 8) + 7.  A row has moved when any lane of its byte of the pass's ballot is set.  All five reductions
// (count, min, max, count, fmax) are independent of the order, so the record is the numpy reduction of the block to the bit.
constexpr int FEET_SUMMARY_WAVES = 4;

__global__ void __launch_bounds__(64 * FEET_SUMMARY_WAVES)
ismpc_a_feet_summary_kernel(const double* __restrict__ feet, const FeetTab tab, const ismpc_a_inst* __restrict__ inst,
                            int rows, int batch, ismpc_a_feet_summary* __restrict__ summary)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * FEET_SUMMARY_WAVES + (threadIdx.x >> 6);        // wave-uniform
    if (b >= batch) return;
    int pl = inst ? inst[b].plan : 0;
    if (pl < 0 || pl >= tab.nplans) pl = 0;                                     // what ismpc_a_feet_fill_inst gave the instance
    const int n = rows * 8, tail = (rows - ISMPC_A_FEET_PAD - 1) * 8;           // the base plan's last row stands behind it (FeetTab)
    const double* f = feet + (size_t)b * n;
    const double* g = tab.base + (size_t)pl * tab.base_rows * 8;
    int moved = 0, first = 0, last = 0, nonfinite = 0;                          // wave-uniform
    double shift = 0.0;                                                         // this lane's column
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        bool differs = false, bad = false;
        if (e < n) {
            const double v = f[e], w = g[e < tail ? e : tail + (e & 7)];
            differs = !(v == w);
            bad = !isfinite(v);
            shift = fmax(shift, fabs(v - w));                                   // fmax: a NaN difference leaves the maximum as it is
        }
        const unsigned long long md = __ballot(differs), mb = __ballot(bad);
        nonfinite += __popcll(mb);
        for (int k = 0; k < 8; ++k) {
            if ((md >> (8 * k)) & 0xffull) {
                const int row = e0 / 8 + k + 1;                                 // 1-based
                ++moved;
                if (first == 0) first = row;
                last = row;
            }
        }
    }
    // x columns are the even lanes, y columns the odd ones: an xor butterfly over the lane bits 1 .. 5 keeps the parity
    for (int d = 2; d < 64; d <<= 1) shift = fmax(shift, __shfl_xor(shift, d));
    const double sy = __shfl(shift, 1);
    if (lane == 0) {
        ismpc_a_feet_summary s;
        s.moved_rows = moved; s.first_moved_row = first; s.last_moved_row = last; s.nonfinite = nonfinite;
        s.max_abs_shift[0] = shift; s.max_abs_shift[1] = sy;
        summary[b] = s;
    }
}

// ---- ismpc_a_foot_trajectories on the device.  The host function's arithmetic, operation for operation: hipcc contracts a * b + c into
// a fused multiply-add in device code by default, the host build has no FMA, and the result is pinned to the bit (the host writer is
// array_equal to the oracle's), so contraction is off for exactly these expressions.  The division is IEEE on both sides.
__device__ __forceinline__ double foot_swing_z(int j)
{
#pragma clang fp contract(off)
    return -0.000032 * j * j + 0.0016 * j;
}
__device__ __forceinline__ double foot_swing_xy(double p, double q, int den, int j)
{
#pragma clang fp contract(off)
    return p + (q - p) / den * j;
}

// One workgroup per (instance, chunk of FOOT_CHUNK_ROWS trajectory rows).  What bounds the kernel is its stores (96 bytes per instance and
// row), so lanes run along the doubles of ONE foot's block: thread t of a pass writes double t of the chunk's rows x 3 doubles of that
// foot, a wavefront 512 contiguous bytes per store.  Trajectory row r of an instance reads the plan rows i = r / step + 1 and i + 1, which
// `step` consecutive rows share: the workgroup copies the plan rows its chunk needs into LDS once (coalesced) and every lane reads its two
// entries from there.  Walk's `cont` cycle (1 .. 8, a foot moves on 2, 4, 6, 8) is ((i - 1) % 8) + 1 for step i: the host function
// starts it at 1 and advances it once per step, so nothing is carried from row to row.
constexpr int FOOT_CHUNK_ROWS = 512;
constexpr int FOOT_THREADS = 256;
constexpr int FOOT_PLAN_ROWS = FOOT_CHUNK_ROWS + 2;                             // a chunk's rows span (FOOT_CHUNK_ROWS - 1) / step + 3 plan rows at the most

__global__ void __launch_bounds__(FOOT_THREADS)
ismpc_a_foot_trajectories_kernel(const FeetTab tab, const ismpc_a_inst* __restrict__ inst, int step_h, const double* __restrict__ feet,
                                 int rows, int sim_duration, int chunks, int batch, double* __restrict__ dst, int32_t* __restrict__ nrows)
{
    extern __shared__ double plan[];                                            // the plan rows of this chunk x 8 (FOOT_PLAN_ROWS at the most)
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;         // uniform
    if (b >= batch) return;
    const int step = inst ? inst[b].step : step_h;
    const int pl = inst ? inst[b].plan : 0;
    // the host function's refusals: the instance writes nothing
    bool ok = step >= 1 && sim_duration >= step && pl >= 0 && pl < tab.nplans;
    int nsteps = 0, n = 0, gait = 0;
    if (ok) {
        nsteps = sim_duration / step; n = nsteps * step; gait = tab.rules[pl].gait;                  // per base plan: 0 = trot, 1 = walk
        ok = nsteps + 1 <= rows && !(gait == 0 && step <= 50);
    }
    if (chunk == 0 && threadIdx.x == 0 && nrows) nrows[b] = ok ? n : -1;
    const int r0 = chunk * FOOT_CHUNK_ROWS;
    if (!ok || r0 >= n) return;
    const int r1 = min(r0 + FOOT_CHUNK_ROWS, n);                                // rows [r0, r1) of the instance
    // plan rows (0-based) r0 / step .. (r1 - 1) / step + 1 <= nsteps <= rows - 1
    const int p0 = r0 / step, p1 = (r1 - 1) / step + 1;
    const double* fp = feet + (size_t)b * rows * 8;
    for (int e = (int)threadIdx.x; e < (p1 + 1 - p0) * 8; e += FOOT_THREADS) plan[e] = fp[p0 * 8 + e];
    __syncthreads();
    const float rstep = 1.0f / (float)step;
    const bool small = sim_duration < (1 << 22);                                // the float quotient below is within 1 of r / step
    const int nd = (r1 - r0) * 3;                                               // doubles of this chunk per foot
    const int swing0 = gait == 0 ? step - 50 : 0;                               // trot: rows 1 .. step - 50 of a step stand still, 50 swing
    const int den = gait == 0 ? 50 : step;
    for (int ft = 0; ft < 4; ++ft) {
        const int col = ft == 0 ? 7 : ft == 1 ? 5 : ft == 2 ? 1 : 3;            // file fl, fr, rl, rr <- plan column FL, FR, BL, BR (1-based x column)
        double* out = dst + (((size_t)b * 4 + ft) * sim_duration + r0) * 3;
        for (int t = threadIdx.x; t < nd; t += FOOT_THREADS) {
            const int rr = t / 3, c = t - 3 * rr;                               // row of the chunk, x / y / z
            const int r = r0 + rr;
            int i0;                                                             // r / step
            if (small) {
                i0 = (int)((float)r * rstep);
                if ((i0 + 1) * step <= r) ++i0;
                if (i0 * step > r) --i0;
            } else {
                i0 = r / step;
            }
            const int i = i0 + 1;                                               // the host loop's step index, 1-based
            const int k = r - i0 * step + 1;                                    // 1 .. step: the row of the step
            const int j = k - swing0;                                           // trot: 1 .. 50 while the pair swings; walk: k
            bool moving;
            if (gait == 0) {
                const bool odd = (i & 1) == 1;                                  // odd steps move BL (1) and FR (5), even ones FL (7) and BR (3)
                moving = j >= 1 && ((col == 1 || col == 5) == odd);
            } else {
                const int cont = ((i - 1) & 7) + 1;
                const int mv = cont == 2 ? 7 : cont == 4 ? 3 : cont == 6 ? 5 : cont == 8 ? 1 : 0;
                moving = col == mv;
            }
            double v;
            if (c == 2) {
                v = moving ? foot_swing_z(j) : 0.0;
            } else {
                const double p = plan[(i0 - p0) * 8 + (col - 1) + c];
                v = moving ? foot_swing_xy(p, plan[(i0 - p0 + 1) * 8 + (col - 1) + c], den, j) : p;
            }
            out[t] = v;
        }
    }
}

}  // namespace
