/*
 * ismpc_a.h -- C ABI of the MI355X-native "Formulation A" ISMPC tick (classic ISMPC with automatic
 * footstep adaptation): the per-tick QP of the reference's MATLAB gait generators, which produced every
 * checked-in trajectory fixture and whose stacked matrices the C++ MPCSolver constructor still allocates
 * (AMR_code_DART/MPCSolver.cpp:34-71).  Reference interfaces replaced (paths relative to the reference root):
 *
 *   ismpc_a_plan            <->  trotting/init_quadruped.m:5-184 , walking/init_quadruped2.m:5-284
 *                                (foot_plan, center = fs_plan)
 *   ismpc_a_create          <->  walking/quad_walk_no_plots.m:6-110 / trotting/quad_as_bip_no_plots.m:6-103
 *                                (constants, A_upd/B_upd, centreline cl_x/cl_y)
 *   ismpc_a_tick_batch_device <-> one iteration of `for j = 1:sim_duration`:
 *                                walking/quad_walk_no_plots.m:127-331,509-559 /
 *                                trotting/quad_as_bip_no_plots.m:116-316,436-479
 *                                (mapping, ZMP / kinematic / stability constraints, quadprog, LIP update,
 *                                 footstep counter + plan shift + centreline rebuild)
 *   ismpc_a_rollout_device  <->  the whole loop, closed on the device
 *
 * The swing-foot re-placement QPs, the foot trajectories and the text wire format are the
 * ismpc_a_*feet* / ismpc_a_foot_trajectories / ismpc_a_write_trajectory_txt entry points further down.
 * Conventions as ismpc.h: plain C, int status, no CPU fallback; every entry point runs on the handle's device and restores
 * the caller's current one.  Launches of one handle must be ordered (the handle owns the copy of the previous state, the
 * work counter and the working-set history that its launches share): use one stream per handle, or order the streams
 * yourself.  When that scratch has to grow inside an asynchronous entry point and the call's stream is not the previous
 * call's, the previous stream is drained first (ismpc_a_reserve avoids both the growth and the wait).
 */
#ifndef ISMPC_A_H
#define ISMPC_A_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-instance status bits (ismpc_a_out.status) */
#define ISMPC_A_ST_OK            0
#define ISMPC_A_ST_X_INFEASIBLE  1    /* the x QP has no feasible point                         */
#define ISMPC_A_ST_Y_INFEASIBLE  2
#define ISMPC_A_ST_OVERFLOW      4    /* the horizon spans more than F-1 step boundaries: the .m file's
                                         `mapping` outgrows its F+1 columns (needs F = ceil(C/step)+1) */
#define ISMPC_A_ST_BAD_INDEX     8    /* j + P beyond the centreline, fc + F beyond the plan, or j outside
                                         the current step [step (fc-1), step fc - 1]               */
#define ISMPC_A_ST_ITER_LIMIT    16   /* active-set iteration limit hit (result is the last iterate)  */
#define ISMPC_A_ST_UNVERIFIED    32   /* set together with X/Y_INFEASIBLE when the flag comes from the final check of
                                         the returned point (a row, a kinematic limit or the stability row is off by
                                         more than 1e-7 relative) and not from the active-set logic itself */

typedef struct ismpc_a_gait {           /* init_quadruped*.m:5-37 */
    int32_t gait;                       /* 0 = trot (init_quadruped.m), 1 = walk (init_quadruped2.m) */
    int32_t n_gait;                     /* N_gait = 100 */
    double  disp_A, phi;                /* step length [m], heading [rad] */
    double  disp_B, disp_C;             /* 0.259394, 0.88 */
    double  disp_i, disp_o, disp_forw;  /* 0.4, 0.4, 0.5 */
} ismpc_a_gait;

typedef struct ismpc_a_params {         /* quad_walk_no_plots.m:15-45,270-271 */
    int32_t C, P, F;                    /* control / preview horizon, footsteps: 100/200/3 (walk), 160/320/3 (trot) */
    int32_t step, ds;                   /* step_duration, dsSamples: 50/30 (walk), 80/50 (trot) */
    int32_t n_gait;                     /* NF */
    double  dt;                         /* mpcTimeStep */
    double  height;                     /* 0.56 */
    double  grav;                       /* 9.8 (the scripts do not use 9.81) */
    double  w;                          /* centroid_size = foot_size = 0.02 */
    double  Qf;                         /* Qfootsteps: 1e9 (walk), 1e7 (trot) */
    double  disp_forw, disp_forw_dummy, disp_L;   /* 0.5, 0.25, (disp_o + disp_i)/2 */
} ismpc_a_params;

/* everything the MATLAB loop carries from tick to tick, per instance (96 bytes) */
typedef struct ismpc_a_state {
    double  x, xd, xz, y, yd, yz;       /* CoM, CoM velocity, ZMP */
    double  cur_x, cur_y;               /* current_xfs, current_yfs */
    double  off_x, off_y;               /* fs_plan(:,c) = base plan + off (quad_walk_no_plots.m:535-536) */
    int32_t fc;                         /* fsCounter, 1-based like the script */
    int32_t j;                          /* tick about to run, 1-based */
    int32_t rebuilt;                    /* 0: initial centreline (:86-99), 1: rebuilt one (:540-549) */
    int32_t reserved;
} ismpc_a_state;

typedef struct ismpc_a_out {            /* 80 bytes */
    double  com_before[2];              /* x_store(j), y_store(j): row j of ComTrajectory_*.txt */
    double  vel_after[2];               /* xd_store(j), yd_store(j): row j of ComVelocity_*.txt */
    double  u0[2];                      /* predicted_xzd(1), predicted_yzd(1) */
    double  f0[2];                      /* predicted_xfs(1), predicted_yfs(1) */
    int32_t status;
    int32_t iters_x, iters_y;           /* work per QP: block warm-start passes + Goldfarb-Idnani steps (+1 for a polish solve) */
    int32_t active;                     /* final working-set sizes: x | y << 16 */
} ismpc_a_out;

/* Per-instance gait parameters for Monte-Carlo / parameter-sweep batches (BASELINE.json configs[4]): every field
 * overrides the handle-wide value of ismpc_a_params for one instance (32 bytes).  The .m scripts hard-code these at
 * quad_walk_no_plots.m:20-45 / quad_as_bip_no_plots.m:16-39; a sweep re-runs the script once per value. */
typedef struct ismpc_a_inst {
    double  height;                     /* CoM height: eta = sqrt(grav / height), A_upd / B_upd, the stability row */
    double  Qf;                         /* Qfootsteps */
    int32_t step, ds;                   /* step_duration, dsSamples */
    int32_t F;                          /* footsteps in this instance's horizon, 1 <= F <= ismpc_a_params.F of the handle */
    int32_t plan;                       /* base plan: 0 = the one given to ismpc_a_create, k = k-th ismpc_a_add_plan; or the index into a plan table */
} ismpc_a_inst;

typedef struct ismpc_a_handle ismpc_a_handle;

void ismpc_a_params_default(int gait, ismpc_a_params* p);
void ismpc_a_gait_default(int gait, double phi, double disp_A, ismpc_a_gait* g);

/* Host: the plan generators.  foot_plan: (n_gait+1) x 8 row-major (BL, BR, FR, FL xy); center: n_gait x 2.
 * Returns the number of foot_plan rows written (n_gait for trot, n_gait+1 for walk) or a negative error. */
int ismpc_a_plan(const ismpc_a_gait* g, double* foot_plan, double* center);

/* center = fs_plan (n_gait x 2 row-major).  disp_C sets the initial state (x = xz = disp_C/2). */
int ismpc_a_create(const ismpc_a_params* p, const double* center, int device, ismpc_a_handle** out);
void ismpc_a_destroy(ismpc_a_handle* h);

/* Optional: size the handle's scratch (copy of the previous state, working-set history, the disturbed rollout's records) for batches up to max_batch now;
 * otherwise it grows inside the asynchronous entry points with stream-ordered allocations on the caller's stream. */
int ismpc_a_reserve(ismpc_a_handle* h, int max_batch);

/* State the scripts start from (quad_walk_no_plots.m:52-62). */
int ismpc_a_initial_state(const ismpc_a_handle* h, double disp_C, ismpc_a_state* st);

/* One tick for every instance.  state is updated in place; push is NULL or batch x 2 impulsive velocity
 * disturbances added before the QP (quad_walk_no_plots.m:134-148); out may be NULL. */
int ismpc_a_tick_batch_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const double* push_dev,
                              ismpc_a_out* out_dev, void* stream);
/* `ticks` ticks, out_traj NULL or ticks x batch records.  Inside a rollout every QP starts from the working set the same
 * instance ended the previous tick with (moved by one sample); the optimum is the same, the route shorter. */
int ismpc_a_rollout_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, int ticks,
                           ismpc_a_out* out_traj_dev, void* stream);
/* Arithmetic type of the QP solve: fp32 = 0 (default) solves in fp64, fp32 = 1 in fp32 -- the dtype BASELINE.json names
 * for its walking-gait and Monte-Carlo configurations.  In both cases the QP is posed relative to the current footstep
 * (every number the solver touches is step-sized), its right-hand sides are formed in fp64 from the fp64 state, and the
 * LIP update of the state (quad_walk_no_plots.m:297-322) is fp64; with fp32 = 1 the active-set iterations, the small
 * linear systems and the returned u0 / f0 carry fp32 rounding (relative CoM error of a tick stays below 1e-6: a tick moves
 * the CoM by B_upd u0 with |B_upd| ~ 1e-6..1e-3).  A QP whose working set pins (nearly) the whole horizon is beyond the
 * fp32 block solve; it is solved by the fp64 instantiation in a small launch (up to 64 workgroups) that follows every fp32 launch on the
 * same stream (about one QP in 30 000 at pushes 1.5x the bench's).  Needs 3 <= F <= 6. */
int ismpc_a_set_precision(ismpc_a_handle* h, int fp32);

/* Introspection (synchronises the stream of the last launch): QPs the last fp32 launch handed to the fp64 re-solve. */
int ismpc_a_last_deferred(ismpc_a_handle* h);

/* The same first guess for caller-driven loops of ismpc_a_tick_batch*_device: enable it when instance i of one call is
 * instance i of the previous one (a wrong guess costs time, never accuracy).  Off by default. */
int ismpc_a_set_warm_history(ismpc_a_handle* h, int enabled);

/* Per-instance gait parameters (one ismpc_a_inst per instance, device pointer).  The handle fixes C, P, dt, w, the
 * kinematic limits and the maximum F; height, Qf, step, ds, F and the base plan come from inst_dev.  An instance
 * whose record is invalid (ds >= step, F out of range, unknown plan, ...) gets ISMPC_A_ST_BAD_INDEX and is left alone. */
int ismpc_a_add_plan(ismpc_a_handle* h, const double* center);      /* returns the plan index (1..3) or a negative error */
int ismpc_a_tick_batch_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev,
                                   const double* push_dev, ismpc_a_out* out_dev, void* stream);
int ismpc_a_rollout_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev,
                                int ticks, ismpc_a_out* out_traj_dev, void* stream);

/* ---- THE WHOLE DECISION and the PREDICTED HORIZON of a tick.
 * ismpc_a_tick_batch_horizon_device is ismpc_a_tick_batch_device (inst_dev NULL) or ismpc_a_tick_batch_inst_device (batch records) with two
 * more outputs.  It serves plain, ismpc_a_add_plan and plan-table handles in either precision and runs whichever kernel the handle
 * dispatches (the wave kernel at every rows-per-lane value, the per-footstep-count launches, the fp32 launch and its fp64 re-solve, the
 * workgroup kernel), in an instantiation that also stores the decision; state, out_dev, the working-set history and the deferred counter
 * are exactly what the plain call produces.
 *
 * dec_dev: [batch][2 axes][C + F] doubles, C and F those of ismpc_a_horizon_shape (F = the handle's maximum).  Per instance and axis
 * u[0 .. C-1] = predicted_xzd(1 .. C), then f[0 .. F-1] = predicted_xfs(1 .. F) as ABSOLUTE footsteps: the scripts' decisionVariables order.
 *   dec[.., 0] is out.u0 and dec[.., C] is out.f0, bit for bit (f[k] = cur + (double)f_rel[k], formed in fp64 as f0 is).
 *   With the fp32 solve the values are the fp32 iterate widened, as u0 / f0 are.
 *   A per-instance record with inst.F < F gets f[inst.F .. F-1] = 0.0 (written, not left as found).
 *   An instance the tick leaves alone (ISMPC_A_ST_BAD_INDEX, ISMPC_A_ST_OVERFLOW): u all 0.0, every f[k] = out.f0 (the current footstep).
 *   An infeasible QP or one that hit the iteration limit returns its last iterate, as u0 does.
 *
 * pred_dev: NULL (no prediction, no further launch) or [batch][2 axes][4][C] doubles: x, xd, xz, zc at samples i = 1 .. C, written by
 * ismpc_a_predict_kernel behind the solver launch(es).
 *   Sample 1 of x, xd, xz is the state the tick just wrote, byte for byte; samples 2 .. C continue the scripts' loop `compute prediction`
 *   (quad_walk_no_plots.m:297-314 with up_to = C) from it: s = A_upd s + B_upd u[i-1] with this instance's A_upd, B_upd, in the expression
 *   order of the tick's own state update.
 *   zc_i is the centre of sample i's ZMP band, w_i g[pf_i] + (1 - w_i) g[pf_i + 1] with g = [cur, f_1 .. f_F] (cur: the PRE-tick current
 *   footstep, f from dec), pf_i and rem_i by the integer rule of the scripts' mapping (pf grows by one when j + i >= step (fc + pf);
 *   rem_i = step (fc + pf_i) - (j + i)) and w_i = 1 when rem_i > ds, else rem_i / ds.  |xz_i - zc_i| <= w / 2 is the ZMP constraint of row i.
 *   Every sample of an instance the tick left alone is a quiet NaN.
 *
 * Returns -1 before the device is touched, ismpc_a_last_error naming the function and the argument: null handle, negative batch, null
 * out_dev, null dec_dev, batch > 0 with a null state_dev.  batch = 0 returns 0.  A closed loop with horizons is the caller-driven loop of
 * this call with ismpc_a_set_warm_history(h, 1). */
int ismpc_a_horizon_shape(const ismpc_a_handle* h, int* C, int* F);
int ismpc_a_tick_batch_horizon_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev,
                                      const ismpc_a_inst* inst_dev,            /* NULL: the handle's parameters; else batch records */
                                      const double* push_dev,                  /* NULL, or batch x 2 */
                                      ismpc_a_out* out_dev,                    /* required */
                                      double* dec_dev,                         /* required: batch x 2 x (C + F) */
                                      double* pred_dev,                        /* NULL, or batch x 2 x 4 x C */
                                      void* stream);

/* ---- PLAN-TABLE handles: any number of base plans, built on the device.
 * ismpc_a_create_plans takes n_plans gait records (host) instead of one centre.  Plan 0 is gaits[0]: everything ismpc_a_create builds
 * from `center` (centreline tables, tails, the plan of the plain launches) is built from the host's ismpc_a_plan(&gaits[0]), so every
 * entry point that takes no ismpc_a_inst behaves exactly as on ismpc_a_create(p, that centre).  All n_plans plans, plan 0 included, are
 * generated by ONE launch on the device into a table the handle owns -- per plan the centre (n_gait x values in the x table, n_gait y
 * values in the y table: the layout the tick kernel's `fs` reads), the foot plan ((n_gait + 1 + ISMPC_A_FEET_PAD) x 8, the last plan row
 * repeated behind the plan) and the foot rules -- bit for bit what ismpc_a_plan writes for the same record.  An instance names its plan
 * in ismpc_a_inst.plan, 0 <= plan < n_plans; any other value gets ISMPC_A_ST_BAD_INDEX and the instance is left alone.
 * Every gaits[k] needs n_gait == p->n_gait and gait 0 (trot) or 1 (walk); the two may mix.  1 <= n_plans <= ISMPC_A_MAX_PLANS: the
 * limit keeps 8 n_plans (the generator's thread index) inside an int32; the table takes 80 n_gait + 616 bytes per plan
 * (8616 bytes at n_gait = 100) and the handle 64 bytes of host memory per plan.
 * Returns -1 before the device is touched, ismpc_a_last_error naming the function and the argument: null p / gaits / out, n_plans < 1
 * or beyond the limit, p->n_gait < 16, a record whose n_gait differs, an unknown gait kind; then ismpc_a_create's own errors.
 * ismpc_a_add_plan and ismpc_a_feet_init_inst_device return -1 on such a handle (the table is the source of plans and foot plans). */
#define ISMPC_A_MAX_PLANS 0x0fffffff
int ismpc_a_create_plans(const ismpc_a_params* p, const ismpc_a_gait* gaits, int n_plans, int device, ismpc_a_handle** out);
/* base plans of the handle: n_plans of ismpc_a_create_plans, or 1 + the ismpc_a_add_plan calls of an ismpc_a_create handle */
int ismpc_a_plans_info(const ismpc_a_handle* h, int* n_plans);
/* milliseconds the generator launch of ismpc_a_create_plans took on the device (HIP events around it); -1: not a plan-table handle */
double ismpc_a_plans_build_ms(const ismpc_a_handle* h);
/* Plan `plan` of a plan-table handle, read back from the device: ismpc_a_plan's outputs (either pointer may be NULL) and its return value. */
int ismpc_a_get_plan(ismpc_a_handle* h, int plan, double* foot_plan, double* center);
/* ismpc_a_initial_state for plan `plan` of a plan-table handle: x = xz = disp_C / 2 of that plan's gait record, the current footstep =
 * the plan's first centre (quad_walk_no_plots.m:52-62). */
int ismpc_a_initial_state_plan(const ismpc_a_handle* h, int plan, ismpc_a_state* st);
/* Host: the transcendental part of ismpc_a_plan -- the clipped step (x, y) and first half step (x, y) of init_quadruped*.m:55-102, in
 * the order xs, ys, xsd, ysd.  ismpc_a_plan and ismpc_a_create_plans both call it; the rest of a plan is additions and the IEEE
 * divisions of the diagonal intersections.  Returns which clip branches ran: 1 = half step lateral, 2 = half step forward,
 * 4 = step lateral, 8 = step forward (or a negative error). */
int ismpc_a_plan_steps(const ismpc_a_gait* g, double steps[4]);

/* DISTURBED closed loop with per-instance summaries: the tick loop of ismpc_a_rollout_device (inst_dev = NULL: the handle's
 * parameters) or ismpc_a_rollout_inst_device (batch records) -- same working-set history, same behaviour on error ticks: the loop goes
 * on -- with the three additions of ismpc_rollout_mc_device (ismpc.h).  Works on every handle those two take, in either precision.  One
 * prologue launch and the solver launch(es) per tick, as there, and one small launch behind the last tick when a summary is asked for.
 * The swing-foot variant, with a feet_dev argument, is ismpc_a_rollout_mc_feet_device further down.
 *
 * PUSHES.  The scripts' impulsive velocity "bang" (quad_walk_no_plots.m:134-148) as a table: pushes_dev holds n_push entries per
 * instance, instance-major (entry k of instance i at [i * n_push + k]).  An entry applies at tick t when its tick == t and no earlier
 * entry of the same instance has a larger tick.  So a table in ascending order applies every entry; several entries with one tick all
 * apply; an entry behind a larger tick is skipped; a negative tick and a tick >= ticks never apply (INT32_MAX pads unused slots, and
 * blocks whatever follows it).  The tick's push is the fp64 sum of its applying entries' dv, in table order from 0.0, and is what
 * ismpc_a_tick_batch_device takes as push_dev: added once to (xd, yd) of the tick's input state, before the QPs.  Ticks count from 0 at
 * THIS call.  dv is not validated: it is a state like any other.
 *
 * TRAJECTORY.  traj_dev is NULL or (ticks / traj_stride) x batch records; tick t is recorded when (t + 1) % traj_stride == 0, in row
 * (t + 1) / traj_stride - 1.  traj_stride = 1 is ismpc_a_rollout_device's layout.
 *
 * SUMMARY.  summary_dev is NULL or batch records, one per instance, over the output records of ALL ticks of the call, recorded or
 * not.  The extrema are taken with fmax: independent of the order and bit-exact against a host reduction (np.fmax) of the stride-1
 * trajectory of the same call.  ticks = 0 gives the empty summary: 0, -1, 0, 0, 0, 0, 0, 0, and 0.0 four times.
 *
 * With n_push = 0, traj_stride = 1 and summary_dev = NULL the call enqueues the launches of ismpc_a_rollout_device /
 * ismpc_a_rollout_inst_device (no push buffer reaches the solver): trajectory and final state are byte-identical.  With pushes it is
 * byte-identical to the caller-driven loop: ismpc_a_set_warm_history(h, 1) on a fresh handle, then `ticks` calls of
 * ismpc_a_tick_batch[_inst]_device, each given a batch x 2 push array (zeros where nothing applies).
 * Returns -1 before the device is touched, ismpc_a_last_error naming the argument: null handle, negative batch or ticks,
 * traj_stride < 1, n_push < 0, n_push > 0 with a null table, batch > 0 with a null state.  The handle-owned scratch (per instance one
 * output record for ticks that only the summary wants, and the tick's push) grows stream-ordered; ismpc_a_reserve sizes it beforehand. */
#define ISMPC_A_ST_ERROR_MASK (ISMPC_A_ST_X_INFEASIBLE | ISMPC_A_ST_Y_INFEASIBLE | ISMPC_A_ST_OVERFLOW | ISMPC_A_ST_BAD_INDEX)

typedef struct ismpc_a_push {            /* 24 bytes */
    int32_t tick;                        /* tick of THIS call, 0 <= tick < ticks */
    int32_t reserved;                    /* 0 */
    double  dv[2];                       /* added to (xd, yd) of the tick's input state, before the QPs */
} ismpc_a_push;

typedef struct ismpc_a_rollout_summary { /* 64 bytes */
    int32_t status_or;                   /* OR of ismpc_a_out.status over all ticks of the call */
    int32_t first_error_tick;            /* first tick with status & ISMPC_A_ST_ERROR_MASK; -1: none */
    int32_t error_ticks;                 /* number of such ticks */
    int32_t iter_limit_ticks;            /* ticks with ISMPC_A_ST_ITER_LIMIT */
    int32_t iters_sum_x, iters_sum_y;    /* sum of iters_x / iters_y over the ticks */
    int32_t max_active_x, max_active_y;  /* max of (active & 0xffff) / (active >> 16) */
    double  max_abs_vel[2];              /* max |vel_after[k]| (fmax) */
    double  max_abs_u0[2];               /* max |u0[k]| (fmax) */
} ismpc_a_rollout_summary;

int ismpc_a_rollout_mc_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev,
                              const ismpc_a_inst* inst_dev,            /* NULL: the handle's parameters; else batch records */
                              int ticks,
                              const ismpc_a_push* pushes_dev, int n_push,  /* batch x n_push, instance-major; NULL with n_push = 0 */
                              int traj_stride, ismpc_a_out* traj_dev,      /* NULL, or (ticks / traj_stride) x batch records */
                              ismpc_a_rollout_summary* summary_dev,        /* NULL, or batch records */
                              void* stream);

/* ---- swing-foot re-placement (the scripts' second quadprog) and the trajectory wire format -------------------
 *   ismpc_a_feet_init_device / ismpc_a_tick_feet_batch_device / ismpc_a_rollout_feet_device
 *        <->  trotting/quad_as_bip_no_plots.m:332-426 + compute_two_feet1.m:1-56
 *             walking/quad_walk_no_plots.m:336-504   + compute_one_feet_walk.m:84-140
 *   ismpc_a_foot_trajectories   <->  quad_as_bip_no_plots.m:482-509 / quad_walk_no_plots.m:562-613
 *   ismpc_a_write_trajectory_txt <-> fprintf(file, '%d %d %d\n', row)   (what Controller.cpp:147-281 reads back)
 * Every instance carries its own foot_plan: feet_dev is batch x ismpc_a_feet_rows(h) x 8 doubles
 * (columns BL, BR, FR, FL xy).                                                                           */
#define ISMPC_A_FEET_PAD 8                           /* feet_dev rows per instance = plan rows + ISMPC_A_FEET_PAD   */
int ismpc_a_feet_rows(const ismpc_a_handle* h);     /* rows per instance in feet_dev, once initialised             */
int ismpc_a_feet_init_device(ismpc_a_handle* h, const ismpc_a_gait* g, const double* foot_plan_host, int rows,
                             int batch, double* feet_dev, void* stream);
/* one tick (as ismpc_a_tick_batch_device) followed by the foot QP of every instance.
 * Lateral limits: a LEFT foot (BL, FL) may move to y in [y_prev - disp_i, y_prev + disp_o], a RIGHT foot (BR, FR) to
 * [y_prev - disp_o, y_prev + disp_i]; every foot to x <= x_prev + disp_forw (y_prev, x_prev: its place in row fc).  All three are halved
 * on the scripts' first ("dummy") steps: trot fc = 1, walk fc = 2 and 4.  Walk re-places a foot only at fc = 2, 4, 6, 8.
 * END OF PLAN.  With `rows` plan rows given to ismpc_a_feet_init*_device (an instance's block is rows + ISMPC_A_FEET_PAD rows, the last
 * plan row repeated in the padding), the foot QP of a tick that ran with footstep counter fc re-places feet when 1 <= fc <= rows - 1 and
 * does nothing for any other fc.  It reads rows fc, fc+1 and writes rows fc+1 .. fc+ISMPC_A_FEET_PAD at the most (1-based), i.e. never
 * outside the instance's rows + ISMPC_A_FEET_PAD rows.  An instance whose tick is flagged ISMPC_A_ST_BAD_INDEX or ISMPC_A_ST_OVERFLOW,
 * or whose base plan index is unknown, keeps its rows untouched.  The oracle (oracle/ismpc_oracle_a.c, orc_a_foot_step) follows the
 * same rule. */
int ismpc_a_tick_feet_batch_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const double* push_dev,
                                   ismpc_a_out* out_dev, double* feet_dev, void* stream);
int ismpc_a_rollout_feet_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, int ticks,
                                ismpc_a_out* out_traj_dev, double* feet_dev, void* stream);
/* The same for batches with per-instance gait parameters (ismpc_a_inst; BASELINE configs[4]): instance b follows the foot
 * rules of its base plan inst[b].plan (trot or walk, heading, lateral limits) and starts from that plan's foot_plan.
 * gaits: one record per base plan of the handle, in the order ismpc_a_create / ismpc_a_add_plan registered them;
 * foot_plans_host: nplans x rows x 8 doubles.  The scripts re-run once per parameter value
 * (trotting/quad_as_bip_no_plots.m:332-426 + compute_two_feet1.m:1-56, walking/quad_walk_no_plots.m:336-504 +
 * compute_one_feet_walk.m:84-140); the foot files of instance b are ismpc_a_foot_trajectories on its rows of feet_dev
 * with its own step_duration.                                                                                          */
int ismpc_a_feet_init_inst_device(ismpc_a_handle* h, const ismpc_a_gait* gaits, const double* foot_plans_host, int rows,
                                  int nplans, int batch, const ismpc_a_inst* inst_dev, double* feet_dev, void* stream);
/* The same start on a plan-table handle (ismpc_a_create_plans): every instance's block is filled from the TABLE's foot plan of its plan
 * (inst_dev NULL: plan 0 for every instance; an unknown index: plan 0, as above); no host foot plan is involved.  rows: plan rows per
 * instance as above, 2 <= rows <= n_gait + 1 (the table holds n_gait + 1 plan rows: a trot plan's last row twice); the block is
 * rows + ISMPC_A_FEET_PAD rows.  Afterwards every feet entry point (tick_feet_batch[_inst], rollout_feet[_inst], rollout_mc_feet,
 * foot_trajectories_device) works on the handle with its documented meaning, for any plan index of the table. */
int ismpc_a_feet_init_plans_device(ismpc_a_handle* h, int rows, int batch, const ismpc_a_inst* inst_dev, double* feet_dev, void* stream);
int ismpc_a_tick_feet_batch_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev,
                                        const double* push_dev, ismpc_a_out* out_dev, double* feet_dev, void* stream);
int ismpc_a_rollout_feet_inst_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev, const ismpc_a_inst* inst_dev,
                                     int ticks, ismpc_a_out* out_traj_dev, double* feet_dev, void* stream);
/* DISTURBED closed loop WITH the swing-foot QPs: ismpc_a_rollout_mc_device (push rule, stride, summary, error behaviour: all as stated
 * there) with ismpc_a_feet_kernel behind the solver launch(es) of every tick, exactly as ismpc_a_tick_feet_batch[_inst]_device launches
 * it -- behind the fp64 re-solve launch of an fp32 handle too.  Works on every handle and launch form ismpc_a_rollout_feet[_inst]_device
 * takes.  feet_dev is batch x ismpc_a_feet_rows(h) x 8, updated in place.
 *   FEET DO NOT FEED BACK.  For the same arguments state_dev, traj_dev and summary_dev are byte-identical to ismpc_a_rollout_mc_device's.
 *   NO DISTURBANCE.  With n_push = 0, traj_stride = 1 and both summaries NULL, state, trajectory and feet_dev are byte-identical to
 *     ismpc_a_rollout_feet_device / ismpc_a_rollout_feet_inst_device.
 *   WITH PUSHES everything, feet_dev included, is byte-identical to the caller-driven loop: ismpc_a_set_warm_history(h, 1) on a fresh
 *     handle, then `ticks` calls of ismpc_a_tick_feet_batch[_inst]_device, each given a batch x 2 push array.
 *   OUTPUT RECORDS.  The foot QP reads the tick's f0 and status, so every tick writes an output record: into its trajectory row when it
 *     has one, else into the handle's scratch records (the ones ismpc_a_rollout_mc_device uses for ticks only the summary wants;
 *     ismpc_a_reserve sizes them).
 *   FEET SUMMARY.  feet_summary_dev is NULL or batch records, written by one launch behind the last tick: every instance's block of
 *     feet_dev, all ismpc_a_feet_rows(h) rows (padding included), against the handle's device copy of the base plans -- plan 0 for a plain
 *     handle, inst[b].plan for a per-instance one, plan 0 when that index is unknown (what ismpc_a_feet_init_inst_device gave the
 *     instance).  It describes the block AS IT STANDS: everything since ismpc_a_feet_init*_device, not only this call.  All five
 *     reductions are independent of the order (count, min, max, fmax), so the record equals a host reduction (np.fmax) of the read-back
 *     block to the bit; a NaN entry is ignored by max_abs_shift and counted by nonfinite and moved_rows.
 * Returns -1 before the device is touched, ismpc_a_last_error naming the function and the argument: negative batch or ticks,
 * traj_stride < 1, n_push < 0, n_push > 0 with a null table, batch > 0 with a null state or a null feet_dev, null handle.  Then, on the
 * handle's device, the messages of ismpc_a_tick_feet_batch[_inst]_device: feet not initialised, a per-instance batch without
 * ismpc_a_feet_init_inst_device.  batch = 0 returns 0; ticks = 0 runs no tick, writes the empty rollout summary and the feet summary of
 * the block as it stands. */
typedef struct ismpc_a_feet_summary {    /* 32 bytes */
    int32_t moved_rows;                  /* rows of the instance's block with any of the 8 entries !(feet == base) */
    int32_t first_moved_row;             /* 1-based; 0: none */
    int32_t last_moved_row;              /* 1-based; 0: none */
    int32_t nonfinite;                   /* entries of the block that are not finite */
    double  max_abs_shift[2];            /* fmax over rows and the four x columns (0,2,4,6) / y columns (1,3,5,7) of |feet - base|, from 0.0 */
} ismpc_a_feet_summary;

int ismpc_a_rollout_mc_feet_device(ismpc_a_handle* h, int batch, ismpc_a_state* state_dev,
                                   const ismpc_a_inst* inst_dev,            /* NULL: the handle's parameters; else batch records */
                                   int ticks,
                                   const ismpc_a_push* pushes_dev, int n_push,
                                   int traj_stride, ismpc_a_out* traj_dev,
                                   ismpc_a_rollout_summary* summary_dev,
                                   double* feet_dev,                        /* batch x ismpc_a_feet_rows(h) x 8, in place */
                                   ismpc_a_feet_summary* feet_summary_dev,  /* NULL, or batch records */
                                   void* stream);

/* Host: the four foot files of one instance.  foot_plan: rows x 8 (as left by the rollout); dst: 4 x n x 3 in the
 * order fl, fr, rl, rr with n = (sim_duration / step) * step rows; returns n. */
int ismpc_a_foot_trajectories(const ismpc_a_gait* g, int step, const double* foot_plan, int rows, int sim_duration, double* dst);
/* Device: the same for a whole batch, bit for bit.  Instance b gets exactly what ismpc_a_foot_trajectories returns for the gait of its
 * base plan (the foot rules given to ismpc_a_feet_init*_device), its own step (inst_dev = NULL: the handle's step and plan 0; else
 * inst[b].step and inst[b].plan), its ismpc_a_feet_rows(h) rows of feet_dev and sim_duration.  dst_dev is batch x 4 x sim_duration x 3,
 * files in the order fl, fr, rl, rr.  With n_b = (sim_duration / step_b) * step_b, rows [0, n_b) of each of the instance's four blocks
 * are written and rows [n_b, sim_duration) are not touched; nrows_dev (NULL, or batch) gets n_b.  Where the host function would refuse
 * (step_b < 1, sim_duration < step_b, n_b / step_b + 1 > ismpc_a_feet_rows(h), a trot plan with step_b <= 50, an unknown plan index)
 * the instance writes nothing and gets nrows_dev[b] = -1; the call itself still returns 0.  The arithmetic is the host function's,
 * operation for operation, with no fused multiply-add.
 * Returns -1 before the device is touched, ismpc_a_last_error naming the function and the argument: null handle, negative batch,
 * sim_duration < 1, batch > 0 with a null feet_dev or dst_dev.  Then the messages of ismpc_a_tick_feet_batch[_inst]_device (feet not
 * initialised, inst_dev without ismpc_a_feet_init_inst_device).  batch = 0 returns 0. */
int ismpc_a_foot_trajectories_device(ismpc_a_handle* h, int batch,
                                     const ismpc_a_inst* inst_dev,           /* NULL: the handle's step and plan 0 */
                                     const double* feet_dev,                 /* batch x ismpc_a_feet_rows(h) x 8 */
                                     int sim_duration,
                                     double* dst_dev,                        /* batch x 4 x sim_duration x 3 */
                                     int32_t* nrows_dev,                     /* NULL, or batch */
                                     void* stream);
/* Host: write n rows of 3 values exactly as MATLAB's fprintf(file, '%d %d %d\n', row) does (integers as %d,
 * everything else as %e).  Returns 0 or a negative error. */
int ismpc_a_write_trajectory_txt(const char* path, const double* rows3, int n);

const char* ismpc_a_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ISMPC_A_H */
