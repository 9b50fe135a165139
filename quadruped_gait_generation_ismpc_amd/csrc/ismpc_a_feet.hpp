// Formulation A, the swing-foot re-placement after a tick (ismpc_a_feet_kernel) and the two kernels that give every instance its
// copy of the base foot plan (ismpc_a_feet_fill, ismpc_a_feet_fill_inst).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "ismpc_a_dev.hpp"

namespace {

// ---- swing-foot re-placement: one thread per instance (closed forms; the 2-/4-variable quadprog is separable, so its
// minimiser is the projection of the target on the box).  trotting/quad_as_bip_no_plots.m:332-426 + compute_two_feet1.m,
// walking/quad_walk_no_plots.m:336-504 + compute_one_feet_walk.m:84-140.
struct FeetParams { int gait, rows; double phi, disp_i, disp_o, disp_forw; };
struct FeetParamsSet { FeetParams p[4]; };           // per base plan (ismpc_a_inst.plan) of an ismpc_a_create handle: host copy of its rules
// What the feet kernels read per base plan, in device memory, for ANY plan index below nplans: the foot rules (FeetParams; its `rows` is
// the table's, the kernels take the instance block's row count as an argument) and the base foot plans, base_rows x 8 doubles per plan.
// An instance block of `rows` rows (plan rows + ISMPC_A_FEET_PAD) starts as base rows 0 .. rows - 9 with the last of them repeated.
struct FeetTab { const FeetParams* rules; const double* base; int nplans, base_rows; };

__device__ __forceinline__ void fixed_diagonal(double fx1, double fy1, double fx2, double fy2, double zx, double zy,
                                               double& m, double& dx, double& dy)
{
    m = (fy2 - fy1) / (fx2 - fx1);
    const double q = fy1 - m * fx1;
    const double xi = (zy + m * zx - q) / (2 * m), yi = m * xi + q;
    dx = zx - xi; dy = zy - yi;
}
__device__ __forceinline__ double clipd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void ismpc_a_feet_kernel(const FeetTab tab, const ismpc_a_inst* __restrict__ inst, const ismpc_a_state* __restrict__ prev,
                                    const ismpc_a_out* __restrict__ out, double* __restrict__ feet, int rows, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    if (out[b].status & (ISMPC_A_ST_BAD_INDEX | ISMPC_A_ST_OVERFLOW)) return;
    int pl = inst ? inst[b].plan : 0;                            // per-instance gait parameters: the foot rules of the instance's base plan
    if (pl < 0 || pl >= tab.nplans) return;
    const FeetParams fpz = tab.rules[pl];
    const int fc = prev[b].fc;                                   // the fsCounter this tick ran with
    if (fc < 1 || fc + 8 >= rows) return;                    // end-of-plan rule of ismpc_a.h: rows fc+1 .. fc+8 stay inside the instance's block
    double* fp = feet + (size_t)b * rows * 8;
#define FPL(r, c) fp[(size_t)((r) - 1) * 8 + ((c) - 1)]
    const double zx = out[b].f0[0], zy = out[b].f0[1];           // predicted_xfs(1), predicted_yfs(1)
    const double di = fpz.disp_i, dob = fpz.disp_o, df = fpz.disp_forw;
    if (fpz.gait == 0) {
        const bool odd = (fc % 2) == 1;
        const int f1 = odd ? 3 : 1, f2 = odd ? 7 : 5, m1 = odd ? 1 : 3, m2 = odd ? 5 : 7;
        double m, dx, dy;
        fixed_diagonal(FPL(fc, f1), FPL(fc, f1 + 1), FPL(fc, f2), FPL(fc, f2 + 1), zx, zy, m, dx, dy);
        const double a1x = FPL(fc + 1, m1), a1y = FPL(fc + 1, m1 + 1), a2x = FPL(fc + 1, m2), a2y = FPL(fc + 1, m2 + 1);
        double x1, y1, x2, y2;
        if (fpz.phi == 3.14159265358979323846 / 2) {
            x1 = a1x; x2 = a2x; y1 = zy - m * (x1 - zx); y2 = zy - m * (x2 - zx);
        } else {
            const double tp = tan(fpz.phi);
            x1 = (zy + m * zx - a1y + tp * a1x) / (tp + m); y1 = tp * (x1 - a1x) + a1y;
            x2 = (zy + m * zx - a2y + tp * a2x) / (tp + m); y2 = tp * (x2 - a2x) + a2y;
        }
        if (dy != 0 || dx != 0) {
            FPL(fc + 1, m1) = x1; FPL(fc + 1, m1 + 1) = y1; FPL(fc + 1, m2) = x2; FPL(fc + 1, m2 + 1) = y2;
            FPL(fc + 1, f1) = FPL(fc, f1); FPL(fc + 1, f1 + 1) = FPL(fc, f1 + 1); FPL(fc + 1, f2) = FPL(fc, f2); FPL(fc + 1, f2 + 1) = FPL(fc, f2 + 1);
        }
        const double lo_ = (fc == 1) ? dob / 2 : dob, li_ = (fc == 1) ? di / 2 : di, lf_ = (fc == 1) ? df / 2 : df;
        // left feet (BL, FL) have their outer side up, right feet (BR, FR) down (quad_as_bip_no_plots.m:393-407): the pair is held by
        // column here, so the first foot is the left one on odd steps (BL) and the right one on even steps (BR)
        const double dn1 = odd ? li_ : lo_, up1 = odd ? lo_ : li_;
        { const double px = FPL(fc, m1), py = FPL(fc, m1 + 1);
          FPL(fc + 1, m1 + 1) = clipd(FPL(fc + 1, m1 + 1), py - dn1, py + up1);
          if (FPL(fc + 1, m1) > px + lf_) FPL(fc + 1, m1) = px + lf_; }
        { const double px = FPL(fc, m2), py = FPL(fc, m2 + 1);
          FPL(fc + 1, m2 + 1) = clipd(FPL(fc + 1, m2 + 1), py - up1, py + dn1);
          if (FPL(fc + 1, m2) > px + lf_) FPL(fc + 1, m2) = px + lf_; }
    } else {
        const int counter = fc;                                  // `counter` (quad_walk_no_plots.m:114,527) starts at 1 and moves with fsCounter
        if (!(counter == 2 || counter == 4 || counter == 6 || counter == 8)) return;
        int mc, a1, a2; bool outer_up;
        if (counter == 2)      { mc = 7; a1 = 1; a2 = 5; outer_up = true; }
        else if (counter == 4) { mc = 3; a1 = 1; a2 = 5; outer_up = false; }
        else if (counter == 6) { mc = 5; a1 = 3; a2 = 7; outer_up = false; }
        else                   { mc = 1; a1 = 3; a2 = 7; outer_up = true; }
        double m, dx, dy;
        fixed_diagonal(FPL(fc, a1), FPL(fc, a1 + 1), FPL(fc, a2), FPL(fc, a2 + 1), zx, zy, m, dx, dy);
        const double xfree = FPL(fc + 1, mc) + dx, yfree = FPL(fc + 1, mc + 1) + dy;
        if (dy != 0 || dx != 0)
            for (int l = 1; l <= 8; ++l) { FPL(fc + l, mc) = xfree; FPL(fc + l, mc + 1) = yfree; }
        const bool dummy = (counter == 2 || counter == 4) && fc <= 4;
        const double lo_ = dummy ? dob / 2 : dob, li_ = dummy ? di / 2 : di, lf_ = dummy ? df / 2 : df;
        const double px = FPL(fc, mc), py = FPL(fc, mc + 1);
        double X1 = FPL(fc + 1, mc), X2 = FPL(fc + 1, mc + 1);
        X2 = outer_up ? clipd(X2, py - li_, py + lo_) : clipd(X2, py - lo_, py + li_);
        if (X1 > px + lf_) X1 = px + lf_;
        if (counter == 8) { for (int l = 1; l <= 8; ++l) FPL(fc + l, mc) = X1; FPL(fc + 1, mc + 1) = X2; }    // :498-503 as written
        else for (int l = 1; l <= 8; ++l) { FPL(fc + l, mc) = X1; FPL(fc + l, mc + 1) = X2; }
    }
#undef FPL
}

__global__ void ismpc_a_feet_fill(const double* __restrict__ base, double* __restrict__ feet, int rows, int batch)
{
    const size_t n = (size_t)batch * rows * 8;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) feet[e] = base[e % ((size_t)rows * 8)];
}
// every instance starts from the foot plan of ITS base plan (FeetTab; inst NULL: plan 0): plan rows 0 .. rows - 9, the last one repeated
__global__ void ismpc_a_feet_fill_inst(const FeetTab tab, const ismpc_a_inst* __restrict__ inst, double* __restrict__ feet, int rows, int batch)
{
    const size_t per = (size_t)rows * 8, n = (size_t)batch * per;
    const size_t last = (size_t)(rows - ISMPC_A_FEET_PAD - 1) * 8;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t b = e / per, k = e - b * per;
        int pl = inst ? inst[b].plan : 0; if (pl < 0 || pl >= tab.nplans) pl = 0;
        feet[e] = tab.base[(size_t)pl * tab.base_rows * 8 + (k < last ? k : last + (k & 7))];
    }
}

}  // namespace
