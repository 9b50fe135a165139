// Formulation A, the plan generators on the device: trotting/init_quadruped.m:5-184 and
// walking/init_quadruped2.m:5-284 for every gait record of a plan-table handle (ismpc_a_create_plans) in one launch, bit for bit what
// the host's ismpc_a_plan writes.
//
// What a plan is made of: the four clipped step scalars (cos, sin, atan: ismpc_a_plan_steps, on the host, four doubles per plan), then
// per foot-plan column a running sum down the rows (a row adds the step to the feet that move in it and copies the others), the
// intersection of the two diagonals of a row for the centre, and walk's copies of the centre.  A column never reads another column, so
// a lane owns one column of one plan: 8 lanes per plan, 8 plans per wavefront, rows in a serial loop.  Row r of the foot plans is then
// one store per wavefront of eight full 64-byte pieces (a plan's rows are 64 bytes, its block a multiple of that), and the centre is
// kept in registers for eight rows -- lane c the row with r % 8 == c -- and stored as 64 contiguous bytes per plan and axis.
//
// Bit equality.  The host function adds and copies in a fixed order per column; this kernel does the same additions in the same
// order (an addition is exact or rounded once, there is nothing to contract).  The diagonal intersection has products and sums: hipcc
// contracts a * b + c into a fused multiply-add in device code by default and the host build has none, so contraction is off for
// exactly those expressions (ismpc_a_feet_files.hpp is the precedent).  The fp64 division is IEEE on both sides.
#pragma once
#include <hip/hip_runtime.h>
#include "ismpc_a_feet.hpp"

namespace {

constexpr int PLAN_GEN_THREADS = 256;                    // 32 plans per workgroup

// rows of a plan's block in the table: n_gait + 1 plan rows (a trot plan has n_gait: its last row stands twice) + the padding
__host__ __device__ constexpr int plan_table_rows(int n_gait) { return n_gait + 1 + ISMPC_A_FEET_PAD; }
// rows ismpc_a_plan writes (its return value): n_gait for trot; walk's eight-row pattern starts at row 6 and runs past n_gait
__host__ __device__ inline int plan_used_rows(int gait, int NG)
{
    if (gait == 0) return NG;
    const int jlast = 6 + 8 * ((NG - 6) / 8);
    return jlast + 7 > NG ? NG + 1 : NG;
}

// ismpc_a_plan's `cross`: the intersection of the diagonals BL-FR and BR-FL of one row (f[0..8): BL, BR, FR, FL xy)
__device__ __forceinline__ void plan_cross(const double* f, double& cx, double& cy)
{
#pragma clang fp contract(off)
    const double m1 = (f[5] - f[1]) / (f[4] - f[0]), b1 = f[1] - m1 * f[0];
    const double m2 = (f[7] - f[3]) / (f[6] - f[2]), b2 = f[3] - m2 * f[2];
    cx = (b2 - b1) / (m1 - m2); cy = m1 * cx + b1;
}

// gaits: the records (device copy), steps: xs, ys, xsd, ysd per plan.  Outputs: the table of DESIGN.md section 2.13.
__global__ void __launch_bounds__(PLAN_GEN_THREADS)
ismpc_a_plan_table_kernel(const ismpc_a_gait* __restrict__ gaits, const double* __restrict__ steps, int n_plans, int NG,
                          double* __restrict__ tab_x, double* __restrict__ tab_y, double* __restrict__ tab_feet, FeetParams* __restrict__ rules)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * PLAN_GEN_THREADS + threadIdx.x;     // 8 n_plans <= INT32_MAX (ISMPC_A_MAX_PLANS)
    const int c = t & 7;                                           // 0-based column: BL x y, BR x y, FR x y, FL x y
    const bool live = (t >> 3) < n_plans;                          // whole groups of 8 lanes; a dead group computes plan n_plans - 1 and stores nothing
    const int p = live ? (t >> 3) : n_plans - 1;
    const ismpc_a_gait g = gaits[p];
    const int axis = c & 1, foot = c >> 1;                         // foot: 0 BL, 1 BR, 2 FR, 3 FL
    const double st = steps[(size_t)p * 4 + axis], sth = steps[(size_t)p * 4 + 2 + axis];
    const int FR_ = plan_table_rows(NG), used = plan_used_rows(g.gait, NG);
    const double v1 = axis == 0 ? (foot >= 2 ? g.disp_C : 0.0) : ((foot == 0 || foot == 3) ? g.disp_B : -g.disp_B);   // row 1
    double* feet = tab_feet + (size_t)p * FR_ * 8 + c;
    double* cxr = tab_x + (size_t)p * NG;
    double* cyr = tab_y + (size_t)p * NG;
    if (live && c == 0) {
        FeetParams f; f.gait = g.gait; f.rows = FR_; f.phi = g.phi; f.disp_i = g.disp_i; f.disp_o = g.disp_o; f.disp_forw = g.disp_forw;
        rules[p] = f;
    }
    // walk: the centre is written for rows 1 .. jmax + 7 (j = 1, 9, ... <= NG - 4), zero behind them
    const int cend = g.gait == 0 ? NG : 1 + 8 * ((NG - 5) / 8) + 7;
    const int lane = threadIdx.x & 63, grp = lane & ~7;
    double v = v1, keep_x = 0.0, keep_y = 0.0, prev_x = 0.0, prev_y = 0.0;
    for (int r = 1; r <= FR_; ++r) {                               // 1-based rows, as the scripts
        if (r >= 2 && r <= used) {
            if (g.gait == 0) {
                if (r == 2) {                                      // the first (half) step: BL and FR
                    if (foot == 0 || foot == 2) v = (c == 0) ? sth : v1 + sth;
                } else {
                    const bool even = (r & 1) == 0;                // even rows move BL and FR, odd rows BR and FL
                    if ((foot == 0 || foot == 2) == even) v = v + st;
                }
            } else if (r <= 5) {                                   // rows 2 .. 5: FL's half step in row 3, BR's in row 5
                if (foot == 3 && r == 3) v = v1 + sth;
                if (foot == 1 && r == 5) v = v + sth;
            } else {
                const int k = (r - 6) & 7;                         // row of the eight-row pattern: FR steps in its row 1, BL 3, FL 5, BR 7
                const int kf = foot == 2 ? 1 : foot == 0 ? 3 : foot == 3 ? 5 : 7;
                if (k == kf) v = v + st;
            }
        }
        if (live) feet[(size_t)(r - 1) * 8] = v;                   // rows behind `used`: the last plan row again
        if (r <= NG) {
            double f[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) f[k] = __shfl(v, grp + k);
            double cx, cy;
            plan_cross(f, cx, cy);
            double ox, oy;
            if (g.gait == 0) { ox = r == 1 ? g.disp_C / 2 : cx; oy = r == 1 ? 0.0 : cy; }
            else if (r > cend) { ox = 0.0; oy = 0.0; }
            else if (r & 1) { ox = cx; oy = cy; }                  // quadruple support: the diagonals
            else { ox = prev_x; oy = prev_y; }                     // triple support: the centre holds
            prev_x = cx; prev_y = cy;
            if (((r - 1) & 7) == c) { keep_x = ox; keep_y = oy; }
            if (((r - 1) & 7) == 7 || r == NG) {
                const int idx = ((r - 1) & ~7) + c;                // 0-based centre row this lane holds
                if (live && idx <= r - 1) { cxr[idx] = keep_x; cyr[idx] = keep_y; }
            }
        }
    }
}

}  // namespace
