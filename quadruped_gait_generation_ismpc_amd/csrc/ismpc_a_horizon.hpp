// Formulation A, the predicted horizon of a tick (ismpc_a_tick_batch_horizon_device): ismpc_a_predict_kernel rolls the
// 3-state LIP forward over the tick's whole decision -- the scripts' loop `compute prediction` (walking/quad_walk_no_plots.m:297-314,
// trotting/quad_as_bip_no_plots.m:287-300) with up_to = C -- and adds the centre of every sample's ZMP band from the adapted footsteps.
// Launched behind the solver launch(es) of the tick on the same stream: it reads what they wrote (dec, out, state) and the handle's
// pre-tick copy of the state.
//
// One lane per (instance, axis) steps the recurrence sequentially: at most 256 dependent steps, and a wavefront scan over the samples
// would need one wavefront per pair -- 2 x batch of them for a few hundred flops each.  What a lane-per-pair layout makes expensive is
// memory: lane l reads u[l][i] and writes four rows [l][i], addresses (C + F) x 8 bytes apart across the wavefront.  So the horizon is cut
// into tiles of HZ_TC samples that go through LDS: global memory is touched in runs of HZ_TC consecutive doubles per pair (a wavefront
// access covers four such runs), LDS is read and written along the other axis.
//   LDS layout: five tiles (u in; x, xd, xz, zc out) of HZ_PAIRS rows with leading dimension HZ_LD = HZ_TC + 1 doubles.  In the stepping
//   phase lane l reads / writes double l * HZ_LD + t: 64-bit accesses bank by (address / 4) mod 64 within a 32-lane half, i.e. by
//   (l * HZ_LD + t) mod 32 in doubles, and an ODD leading dimension maps the 32 lanes of a half onto the 32 distinct residues: no
//   conflict.  In words the stride is 2 HZ_LD = 34, not a multiple of four (DESIGN.md section 7 measured 41 % conflict cycles on a
//   stride-4-word pattern).  In the transfer phases 16 consecutive lanes touch 16 consecutive doubles of one row: conflict-free as well.
#pragma once
#include <hip/hip_runtime.h>
#include "ismpc_a_dev.hpp"

namespace {

constexpr int HZ_PAIRS = 64;              // (instance, axis) pairs per workgroup: one wavefront, one lane each
constexpr int HZ_TC = 16;                 // samples per tile: runs of 128 bytes in global memory
constexpr int HZ_LD = HZ_TC + 1;          // leading dimension of a tile, in doubles (odd)
constexpr int HZ_GL = ismpc_a::MAXF + 1;  // g = [cur, f_1 .. f_F] per pair (odd as well)

// pred: [batch][2 axes][4][C] doubles -- x, xd, xz, zc at samples 1 .. C (include/ismpc_a.h).  inst / pre: NULL on a plain launch.
__global__ __launch_bounds__(HZ_PAIRS)
void ismpc_a_predict_kernel(const ismpc_a::DevA c, const ismpc_a_state* __restrict__ prev, const ismpc_a_state* __restrict__ state,
                            const ismpc_a_inst* __restrict__ inst, const ismpc_a::PiPre* __restrict__ pre, const ismpc_a_out* __restrict__ out,
                            const double* __restrict__ dec, double* __restrict__ pred, int batch)
{
    __shared__ double tu[HZ_PAIRS * HZ_LD], tx[HZ_PAIRS * HZ_LD], tv[HZ_PAIRS * HZ_LD], tz[HZ_PAIRS * HZ_LD], tc[HZ_PAIRS * HZ_LD];
    __shared__ double gl[HZ_PAIRS * HZ_GL];
    const int lane = threadIdx.x;
    const int C = c.C, F = c.F;
    const long long npairs = 2ll * batch, pair0 = (long long)blockIdx.x * HZ_PAIRS, pair = pair0 + lane;
    const size_t dstride = (size_t)(C + F);

    // ---- this lane's pair: the pre-tick record (cur, j, fc), the gait parameters, the LIP matrices, sample 1
    bool left = true;                                      // the tick left the instance alone (or no pair): every sample a quiet NaN
    int j = 1, fc = 1, step = 2, ds = 1;
    double p = 0.0, v = 0.0, z = 0.0;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a10 = 0.0, a11 = 0.0, a12 = 0.0, a20 = 0.0, a21 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (pair < npairs) {
        const int i = (int)(pair >> 1), axis = (int)(pair & 1);
        left = (out[i].status & (ISMPC_A_ST_BAD_INDEX | ISMPC_A_ST_OVERFLOW)) != 0;
        const ismpc_a_state* sb = prev + i;
        j = sb->j; fc = sb->fc;
        gl[lane * HZ_GL] = axis == 0 ? sb->cur_x : sb->cur_y;
        const double* fq = dec + (size_t)pair * dstride + C;
        for (int k = 1; k < HZ_GL; ++k) gl[lane * HZ_GL + k] = k <= F ? fq[k - 1] : 0.0;
        const ismpc_a_state* sa = state + i;
        p = axis == 0 ? sa->x : sa->y; v = axis == 0 ? sa->xd : sa->yd; z = axis == 0 ? sa->xz : sa->yz;
        if (inst) {
            // A_upd, B_upd of this instance's eta, entry by entry what the tick's own update multiplies with (ismpc_a_wave.hpp)
            step = inst[i].step; ds = inst[i].ds;
            const double ch = pre[i].ch, sh = pre[i].sh, she = pre[i].sh_eta, eta = pre[i].eta;
            a00 = ch; a01 = she; a02 = 1 - ch; b0 = c.dt - she;
            a10 = eta * sh; a11 = ch; a12 = -eta * sh; b1 = 1 - ch;
            a20 = 0.0; a21 = 0.0; a22 = 1.0; b2 = c.dt;
        } else {
            step = c.step; ds = c.ds;
            a00 = c.Au[0]; a01 = c.Au[1]; a02 = c.Au[2]; a10 = c.Au[3]; a11 = c.Au[4]; a12 = c.Au[5]; a20 = c.Au[6]; a21 = c.Au[7]; a22 = c.Au[8];
            b0 = c.Bu[0]; b1 = c.Bu[1]; b2 = c.Bu[2];
        }
    }
    const double qnan = __builtin_nan("");
    int pf = 0;                                            // first mapped footstep of the sample, by the integer rule of the mapping
    // the transfer phases: element e = it * 64 + lane of a tile is (row e / HZ_TC, column e % HZ_TC)
    const int trow = lane / HZ_TC, tcol = lane % HZ_TC;
    constexpr int ROWS_PER_IT = HZ_PAIRS / HZ_TC;

    for (int c0 = 0; c0 < C; c0 += HZ_TC) {
        // ---- u[c0 .. c0 + HZ_TC) of every pair into LDS
        for (int it = 0; it < HZ_TC; ++it) {
            const int row = it * ROWS_PER_IT + trow;
            const long long pr = pair0 + row;
            if (pr < npairs && c0 + tcol < C) tu[row * HZ_LD + tcol] = dec[(size_t)pr * dstride + c0 + tcol];
        }
        __syncthreads();
        // ---- samples c0 + 1 .. c0 + HZ_TC of this lane's pair
        for (int t = 0; t < HZ_TC; ++t) {
            const int s = c0 + t;                          // sample s + 1
            if (s >= C) break;
            if (s > 0) {
                // s = A_upd s + B_upd u[s]: the tick's own expression order
                const double u = tu[lane * HZ_LD + t];
                const double np_ = (a00 * p + a01 * v + a02 * z) + b0 * u;
                const double nv_ = (a10 * p + a11 * v + a12 * z) + b1 * u;
                const double nz_ = (a20 * p + a21 * v + a22 * z) + b2 * u;
                p = np_; v = nv_; z = nz_;
            }
            // centre of the sample's band: w g[pf] + (1 - w) g[pf + 1], g = [cur, f_1 .. f_F]
            const int i1 = s + 1;
            if (j + i1 >= step * (fc + pf)) ++pf;
            const int rem = step * (fc + pf) - (j + i1);
            const double w = rem > ds ? 1.0 : (double)rem / (double)ds;
            const int k0 = pf < F ? pf : F, k1 = pf + 1 < F ? pf + 1 : F;
            const double zc = w * gl[lane * HZ_GL + k0] + (1.0 - w) * gl[lane * HZ_GL + k1];
            tx[lane * HZ_LD + t] = left ? qnan : p;
            tv[lane * HZ_LD + t] = left ? qnan : v;
            tz[lane * HZ_LD + t] = left ? qnan : z;
            tc[lane * HZ_LD + t] = left ? qnan : zc;
        }
        __syncthreads();
        // ---- the four rows of every pair out of LDS
        for (int it = 0; it < HZ_TC; ++it) {
            const int row = it * ROWS_PER_IT + trow;
            const long long pr = pair0 + row;
            if (pr < npairs && c0 + tcol < C) {
                double* dst = pred + (size_t)pr * 4 * (size_t)C + c0 + tcol;
                const int e = row * HZ_LD + tcol;
                dst[0] = tx[e]; dst[(size_t)C] = tv[e]; dst[2 * (size_t)C] = tz[e]; dst[3 * (size_t)C] = tc[e];
            }
        }
        // (the next tile's u is written before the barrier that precedes the next stepping phase, and nothing reads tu in between)
    }
}

}  // namespace
