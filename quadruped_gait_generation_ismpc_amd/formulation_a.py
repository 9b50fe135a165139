"""Host-side mirror of the reference's MATLAB gait generators ("Formulation A") over the C ABI of
include/ismpc_a.h: plan generators (init_quadruped*.m) and the per-tick ISMPC QP with footstep adaptation
(quad_walk_no_plots.m / quad_as_bip_no_plots.m loop body).  All compute is HIP; nothing is solved in Python."""
import ctypes as C
import os

import numpy as np

from . import _lib

TROT, WALK = 0, 1
ST_X_INFEASIBLE, ST_Y_INFEASIBLE, ST_OVERFLOW, ST_BAD_INDEX, ST_ITER_LIMIT, ST_UNVERIFIED = 1, 2, 4, 8, 16, 32


class GaitA(C.Structure):
    _fields_ = [("gait", C.c_int32), ("n_gait", C.c_int32), ("disp_A", C.c_double), ("phi", C.c_double),
                ("disp_B", C.c_double), ("disp_C", C.c_double), ("disp_i", C.c_double), ("disp_o", C.c_double),
                ("disp_forw", C.c_double)]


class ParamsA(C.Structure):
    _fields_ = [("C", C.c_int32), ("P", C.c_int32), ("F", C.c_int32), ("step", C.c_int32), ("ds", C.c_int32),
                ("n_gait", C.c_int32), ("dt", C.c_double), ("height", C.c_double), ("grav", C.c_double),
                ("w", C.c_double), ("Qf", C.c_double), ("disp_forw", C.c_double), ("disp_forw_dummy", C.c_double),
                ("disp_L", C.c_double)]


STATE_A = np.dtype([("x", "<f8"), ("xd", "<f8"), ("xz", "<f8"), ("y", "<f8"), ("yd", "<f8"), ("yz", "<f8"),
                    ("cur_x", "<f8"), ("cur_y", "<f8"), ("off_x", "<f8"), ("off_y", "<f8"),
                    ("fc", "<i4"), ("j", "<i4"), ("rebuilt", "<i4"), ("reserved", "<i4")], align=False)
OUT_A = np.dtype([("com_before", "<f8", 2), ("vel_after", "<f8", 2), ("u0", "<f8", 2), ("f0", "<f8", 2),
                  ("status", "<i4"), ("iters_x", "<i4"), ("iters_y", "<i4"), ("active", "<i4")], align=False)
INST_A = np.dtype([("height", "<f8"), ("Qf", "<f8"), ("step", "<i4"), ("ds", "<i4"), ("F", "<i4"), ("plan", "<i4")], align=False)
assert STATE_A.itemsize == 96 and OUT_A.itemsize == 80 and INST_A.itemsize == 32
# the disturbed closed loop (ismpc_a_rollout_mc_device): one push-table entry, one per-instance summary
PUSH_A = np.dtype([("tick", "<i4"), ("reserved", "<i4"), ("dv", "<f8", 2)], align=False)
ROLLOUT_SUMMARY_A = np.dtype([("status_or", "<i4"), ("first_error_tick", "<i4"), ("error_ticks", "<i4"), ("iter_limit_ticks", "<i4"),
                              ("iters_sum_x", "<i4"), ("iters_sum_y", "<i4"), ("max_active_x", "<i4"), ("max_active_y", "<i4"),
                              ("max_abs_vel", "<f8", 2), ("max_abs_u0", "<f8", 2)], align=False)
assert PUSH_A.itemsize == 24 and ROLLOUT_SUMMARY_A.itemsize == 64
ST_ERROR_MASK_A = ST_X_INFEASIBLE | ST_Y_INFEASIBLE | ST_OVERFLOW | ST_BAD_INDEX      # ISMPC_A_ST_ERROR_MASK = 15
# the disturbed closed loop with the swing-foot QPs (ismpc_a_rollout_mc_feet_device): an instance's foot plan block against its base plan
FEET_SUMMARY_A = np.dtype([("moved_rows", "<i4"), ("first_moved_row", "<i4"), ("last_moved_row", "<i4"), ("nonfinite", "<i4"),
                           ("max_abs_shift", "<f8", 2)], align=False)
assert FEET_SUMMARY_A.itemsize == 32

EXPORTS_A = ["ismpc_a_params_default", "ismpc_a_gait_default", "ismpc_a_plan", "ismpc_a_create", "ismpc_a_destroy",
             "ismpc_a_initial_state", "ismpc_a_tick_batch_device", "ismpc_a_rollout_device", "ismpc_a_last_error",
             "ismpc_a_feet_rows", "ismpc_a_feet_init_device", "ismpc_a_tick_feet_batch_device",
             "ismpc_a_rollout_feet_device", "ismpc_a_foot_trajectories", "ismpc_a_write_trajectory_txt",
             "ismpc_a_add_plan", "ismpc_a_tick_batch_inst_device", "ismpc_a_rollout_inst_device", "ismpc_a_set_warm_history", "ismpc_a_reserve", "ismpc_a_set_precision",
             "ismpc_a_last_deferred", "ismpc_a_feet_init_inst_device", "ismpc_a_tick_feet_batch_inst_device",
             "ismpc_a_rollout_feet_inst_device", "ismpc_a_rollout_mc_device", "ismpc_a_rollout_mc_feet_device",
             "ismpc_a_foot_trajectories_device", "ismpc_a_create_plans", "ismpc_a_plans_info", "ismpc_a_plans_build_ms", "ismpc_a_get_plan",
             "ismpc_a_initial_state_plan", "ismpc_a_plan_steps", "ismpc_a_feet_init_plans_device",
             "ismpc_a_horizon_shape", "ismpc_a_tick_batch_horizon_device"]
MAX_PLANS = 0x0fffffff  # ISMPC_A_MAX_PLANS
HAVE_F32 = True        # the QP solve also exists in fp32 (GaitGenerator(..., precision="f32"))
FEET_PAD = 8

_bound = False


def _l():
    global _bound
    lib = _lib.load()
    if not _bound:
        vp, ci, cd = C.c_void_p, C.c_int, C.c_double
        lib.ismpc_a_params_default.argtypes = [ci, C.POINTER(ParamsA)]; lib.ismpc_a_params_default.restype = None
        lib.ismpc_a_gait_default.argtypes = [ci, cd, cd, C.POINTER(GaitA)]; lib.ismpc_a_gait_default.restype = None
        lib.ismpc_a_plan.argtypes = [C.POINTER(GaitA), vp, vp]; lib.ismpc_a_plan.restype = ci
        lib.ismpc_a_create.argtypes = [C.POINTER(ParamsA), vp, ci, C.POINTER(vp)]; lib.ismpc_a_create.restype = ci
        lib.ismpc_a_destroy.argtypes = [vp]; lib.ismpc_a_destroy.restype = None
        lib.ismpc_a_initial_state.argtypes = [vp, cd, vp]; lib.ismpc_a_initial_state.restype = ci
        lib.ismpc_a_tick_batch_device.argtypes = [vp, ci, vp, vp, vp, vp]; lib.ismpc_a_tick_batch_device.restype = ci
        lib.ismpc_a_rollout_device.argtypes = [vp, ci, vp, ci, vp, vp]; lib.ismpc_a_rollout_device.restype = ci
        lib.ismpc_a_last_error.argtypes = []; lib.ismpc_a_last_error.restype = C.c_char_p
        lib.ismpc_a_feet_rows.argtypes = [vp]; lib.ismpc_a_feet_rows.restype = ci
        lib.ismpc_a_feet_init_device.argtypes = [vp, C.POINTER(GaitA), vp, ci, ci, vp, vp]; lib.ismpc_a_feet_init_device.restype = ci
        lib.ismpc_a_tick_feet_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, vp]; lib.ismpc_a_tick_feet_batch_device.restype = ci
        lib.ismpc_a_rollout_feet_device.argtypes = [vp, ci, vp, ci, vp, vp, vp]; lib.ismpc_a_rollout_feet_device.restype = ci
        lib.ismpc_a_foot_trajectories.argtypes = [C.POINTER(GaitA), ci, vp, ci, ci, vp]; lib.ismpc_a_foot_trajectories.restype = ci
        lib.ismpc_a_write_trajectory_txt.argtypes = [C.c_char_p, vp, ci]; lib.ismpc_a_write_trajectory_txt.restype = ci
        lib.ismpc_a_set_warm_history.argtypes = [vp, ci]; lib.ismpc_a_set_warm_history.restype = ci
        lib.ismpc_a_add_plan.argtypes = [vp, vp]; lib.ismpc_a_add_plan.restype = ci
        lib.ismpc_a_tick_batch_inst_device.argtypes = [vp, ci, vp, vp, vp, vp, vp]; lib.ismpc_a_tick_batch_inst_device.restype = ci
        lib.ismpc_a_rollout_inst_device.argtypes = [vp, ci, vp, vp, ci, vp, vp]; lib.ismpc_a_rollout_inst_device.restype = ci
        lib.ismpc_a_reserve.argtypes = [vp, ci]; lib.ismpc_a_reserve.restype = ci
        lib.ismpc_a_set_precision.argtypes = [vp, ci]; lib.ismpc_a_set_precision.restype = ci
        lib.ismpc_a_last_deferred.argtypes = [vp]; lib.ismpc_a_last_deferred.restype = ci
        lib.ismpc_a_feet_init_inst_device.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, vp]; lib.ismpc_a_feet_init_inst_device.restype = ci
        lib.ismpc_a_tick_feet_batch_inst_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]; lib.ismpc_a_tick_feet_batch_inst_device.restype = ci
        lib.ismpc_a_rollout_feet_inst_device.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]; lib.ismpc_a_rollout_feet_inst_device.restype = ci
        lib.ismpc_a_rollout_mc_device.argtypes = [vp, ci, vp, vp, ci, vp, ci, ci, vp, vp, vp]; lib.ismpc_a_rollout_mc_device.restype = ci
        lib.ismpc_a_rollout_mc_feet_device.argtypes = [vp, ci, vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, vp]; lib.ismpc_a_rollout_mc_feet_device.restype = ci
        lib.ismpc_a_foot_trajectories_device.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp]; lib.ismpc_a_foot_trajectories_device.restype = ci
        lib.ismpc_a_create_plans.argtypes = [C.POINTER(ParamsA), vp, ci, ci, C.POINTER(vp)]; lib.ismpc_a_create_plans.restype = ci
        lib.ismpc_a_plans_info.argtypes = [vp, C.POINTER(ci)]; lib.ismpc_a_plans_info.restype = ci
        lib.ismpc_a_plans_build_ms.argtypes = [vp]; lib.ismpc_a_plans_build_ms.restype = cd
        lib.ismpc_a_get_plan.argtypes = [vp, ci, vp, vp]; lib.ismpc_a_get_plan.restype = ci
        lib.ismpc_a_initial_state_plan.argtypes = [vp, ci, vp]; lib.ismpc_a_initial_state_plan.restype = ci
        lib.ismpc_a_plan_steps.argtypes = [C.POINTER(GaitA), vp]; lib.ismpc_a_plan_steps.restype = ci
        lib.ismpc_a_feet_init_plans_device.argtypes = [vp, ci, ci, vp, vp, vp]; lib.ismpc_a_feet_init_plans_device.restype = ci
        lib.ismpc_a_horizon_shape.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]; lib.ismpc_a_horizon_shape.restype = ci
        lib.ismpc_a_tick_batch_horizon_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]; lib.ismpc_a_tick_batch_horizon_device.restype = ci
        _bound = True
    return lib


class IsmpcAError(RuntimeError):
    pass


def default_params(gait, **over):
    p = ParamsA()
    _l().ismpc_a_params_default(int(gait), C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_gait(gait, phi, disp_A):
    g = GaitA()
    _l().ismpc_a_gait_default(int(gait), float(phi), float(disp_A), C.byref(g))
    return g


def plan(g):
    """init_quadruped.m / init_quadruped2.m: (foot_plan [rows, 8], center = fs_plan [n_gait, 2])."""
    fp = np.zeros((g.n_gait + 1, 8)); ce = np.zeros((g.n_gait, 2))
    used = _l().ismpc_a_plan(C.byref(g), fp.ctypes.data_as(C.c_void_p), ce.ctypes.data_as(C.c_void_p))
    if used < 0:
        raise IsmpcAError(_l().ismpc_a_last_error().decode())
    return fp[:used].copy(), ce


CLIP_HALF_LATERAL, CLIP_HALF_FORWARD, CLIP_STEP_LATERAL, CLIP_STEP_FORWARD = 1, 2, 4, 8


def plan_steps(g):
    """The clipped step and first half step of a plan (ismpc_a_plan_steps): (array [xs, ys, xsd, ysd], the CLIP_* branches that ran)."""
    s = np.zeros(4)
    rc = _l().ismpc_a_plan_steps(C.byref(g), s.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise IsmpcAError(_l().ismpc_a_last_error().decode())
    return s, rc


def foot_trajectories(g, step, foot_plan, sim_duration=2000):
    """Host: the four foot files (fl, fr, rl, rr) of one instance, [4, rows, 3]  (quad_*_no_plots.m foot writers)."""
    fp = np.ascontiguousarray(foot_plan, dtype=np.float64)
    n = (sim_duration // step) * step
    dst = np.zeros((4, n, 3))
    rc = _l().ismpc_a_foot_trajectories(C.byref(g), int(step), fp.ctypes.data_as(C.c_void_p), fp.shape[0], int(sim_duration),
                                        dst.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise IsmpcAError(_l().ismpc_a_last_error().decode())
    return dst


def write_trajectory_txt(path, rows3):
    """The text wire format the DART controller reads back (Controller.cpp:147-281): MATLAB's '%d %d %d\n'."""
    a = np.ascontiguousarray(rows3, dtype=np.float64).reshape(-1, 3)
    rc = _l().ismpc_a_write_trajectory_txt(os.fsencode(path), a.ctypes.data_as(C.c_void_p), a.shape[0])
    if rc != 0:
        raise IsmpcAError(_l().ismpc_a_last_error().decode())


class GaitGenerator:
    """The MATLAB loop `for j = 1:sim_duration` (quad_walk_no_plots.m:127 / quad_as_bip_no_plots.m:116),
    batched: every instance carries its own (state, footstep counter, plan shift)."""

    def __init__(self, params, center, device=0, precision="f64"):
        """precision: arithmetic type of the QP solve, "f64" (default) or "f32" (ismpc_a_set_precision); the state, the
        right-hand sides of the QP and the LIP update are fp64 either way."""
        if precision not in ("f64", "f32"):
            raise ValueError("precision must be 'f64' or 'f32'")
        self.precision = precision
        self.params = params
        self.center = np.ascontiguousarray(center, dtype=np.float64)
        h = C.c_void_p()
        rc = _l().ismpc_a_create(C.byref(params), self.center.ctypes.data_as(C.c_void_p), int(device), C.byref(h))
        if rc != 0:
            raise IsmpcAError(f"ismpc_a_create: {rc}: {_l().ismpc_a_last_error().decode()}")
        self._h = h
        if _l().ismpc_a_set_precision(self._h, 1 if precision == "f32" else 0) != 0:
            msg = _l().ismpc_a_last_error().decode(); self.close()
            raise IsmpcAError(msg)

    @classmethod
    def from_gaits(cls, params, gaits, device=0, precision="f64"):
        """A plan-table handle (ismpc_a_create_plans): one base plan per GaitA record of `gaits`, all of them built on the device; an
        instance names its plan in INST_A["plan"].  Plan 0 is gaits[0]: without INST_A records the generator is GaitGenerator(params,
        plan(gaits[0])[1]).  add_plan and feet_init_inst_torch are refused; feet start with feet_init_plans_torch."""
        if precision not in ("f64", "f32"):
            raise ValueError("precision must be 'f64' or 'f32'")
        gaits = list(gaits)
        self = cls.__new__(cls)
        self.precision, self.params, self._h = precision, params, None
        self.gaits = gaits
        ga = (GaitA * max(len(gaits), 1))(*gaits)
        h = C.c_void_p()
        rc = _l().ismpc_a_create_plans(C.byref(params), C.cast(ga, C.c_void_p), len(gaits), int(device), C.byref(h))
        if rc != 0:
            raise IsmpcAError(f"ismpc_a_create_plans: {rc}: {_l().ismpc_a_last_error().decode()}")
        self._h = h
        self.center = plan(gaits[0])[1]
        if _l().ismpc_a_set_precision(self._h, 1 if precision == "f32" else 0) != 0:
            msg = _l().ismpc_a_last_error().decode(); self.close()
            raise IsmpcAError(msg)
        return self

    @property
    def n_plans(self):
        """Base plans of the handle: the table's count, or 1 + the add_plan calls."""
        n = C.c_int(0)
        if _l().ismpc_a_plans_info(self._h, C.byref(n)) != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return n.value

    @property
    def plans_build_ms(self):
        """Milliseconds the generator launch of from_gaits took on the device."""
        return _l().ismpc_a_plans_build_ms(self._h)

    def get_plan(self, k):
        """Plan k of a plan-table generator, read back from the device: (foot_plan [rows, 8], center [n_gait, 2]) as plan() returns them."""
        ng = self.params.n_gait
        fp = np.zeros((ng + 1, 8)); ce = np.zeros((ng, 2))
        used = _l().ismpc_a_get_plan(self._h, int(k), fp.ctypes.data_as(C.c_void_p), ce.ctypes.data_as(C.c_void_p))
        if used < 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return fp[:used].copy(), ce

    def initial_state_plan(self, k, batch=1):
        """The state the scripts start from for plan k's gait record (ismpc_a_initial_state_plan)."""
        st = np.zeros(1, dtype=STATE_A)
        if _l().ismpc_a_initial_state_plan(self._h, int(k), st.ctypes.data_as(C.c_void_p)) != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return np.repeat(st, batch)

    def feet_init_plans_torch(self, inst_u8, rows=None):
        """Plan-table generators: every instance's foot plan block from the table's foot plan of its plan (ismpc_a_feet_init_plans_device;
        inst_u8: CUDA uint8 [batch, 32] INST_A records).  rows: plan rows per instance, default what feet_init_inst_torch takes for the
        same gaits (n_gait + 1 when a walk plan is among them, else n_gait).  Returns float64 tensor [batch, rows + FEET_PAD, 8]."""
        import torch
        assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.dim() == 2 and inst_u8.shape[1] == 32 and inst_u8.is_contiguous()
        if rows is None:
            rows = self.params.n_gait + (1 if any(g.gait == WALK for g in getattr(self, "gaits", [])) else 0)
        b = inst_u8.shape[0]
        feet = torch.empty((b, int(rows) + FEET_PAD, 8), dtype=torch.float64, device=inst_u8.device)
        stream = torch.cuda.current_stream(inst_u8.device).cuda_stream
        rc = _l().ismpc_a_feet_init_plans_device(self._h, int(rows), b, C.c_void_p(inst_u8.data_ptr()), C.c_void_p(feet.data_ptr()),
                                                 C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return feet

    def close(self):
        if getattr(self, "_h", None) and _l is not None:
            _l().ismpc_a_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def initial_state(self, disp_C=0.88, batch=1):
        st = np.zeros(1, dtype=STATE_A)
        rc = _l().ismpc_a_initial_state(self._h, float(disp_C), st.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return np.repeat(st, batch)

    def tick_device(self, batch, state_ptr, push_ptr=None, out_ptr=None, stream=None):
        rc = _l().ismpc_a_tick_batch_device(self._h, int(batch), C.c_void_p(state_ptr),
                                            C.c_void_p(push_ptr) if push_ptr else None,
                                            C.c_void_p(out_ptr) if out_ptr else None,
                                            C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    def horizon_shape(self):
        """(C, F) of the handle (ismpc_a_horizon_shape): a tick's decision is 2 x (C + F) doubles per instance, its prediction 2 x 4 x C."""
        c, f = C.c_int(0), C.c_int(0)
        if _l().ismpc_a_horizon_shape(self._h, C.byref(c), C.byref(f)) != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return c.value, f.value

    def tick_horizon_device(self, batch, state_ptr, out_ptr, dec_ptr, pred_ptr=None, push_ptr=None, inst_ptr=None, stream=None):
        """ismpc_a_tick_batch_horizon_device on raw device pointers: the tick with its whole decision (dec_ptr: batch x 2 x (C + F) doubles)
        and, with pred_ptr, the predicted horizon (batch x 2 x 4 x C doubles: x, xd, xz, zc at samples 1 .. C)."""
        opt = lambda p: C.c_void_p(p) if p else None
        rc = _l().ismpc_a_tick_batch_horizon_device(self._h, int(batch), opt(state_ptr), opt(inst_ptr), opt(push_ptr), opt(out_ptr), opt(dec_ptr),
                                                    opt(pred_ptr), opt(stream))
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    def tick_horizon_torch(self, state_u8, push=None, inst_u8=None, want_pred=True):
        """One tick (tick_torch, or tick_inst_torch with inst_u8) that also returns every QP's whole decision and the predicted horizon.
        state_u8: CUDA uint8 [batch, 96], updated in place; push: None or CUDA float64 [batch, 2]; inst_u8: None or CUDA uint8 [batch, 32].
        Returns (out_u8 [batch, 80], dec float64 [batch, 2, C + F], pred float64 [batch, 2, 4, C] or None) on the state's device.  dec: the
        ZMP velocities u[0 .. C-1] then the absolute footsteps f[0 .. F-1] per axis; pred: x, xd, xz and the band centre zc at samples
        1 .. C (NaN for an instance the tick left alone)."""
        import torch
        b = state_u8.shape[0]
        assert state_u8.is_cuda and state_u8.dtype == torch.uint8 and state_u8.shape[1] == 96 and state_u8.is_contiguous()
        if inst_u8 is not None:
            assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.shape == (b, 32) and inst_u8.is_contiguous() and inst_u8.device == state_u8.device
        if push is not None:
            assert push.is_cuda and push.dtype == torch.float64 and tuple(push.shape) == (b, 2) and push.is_contiguous() and push.device == state_u8.device
        c, f = self.horizon_shape()
        out = torch.empty((b, 80), dtype=torch.uint8, device=state_u8.device)
        dec = torch.empty((b, 2, c + f), dtype=torch.float64, device=state_u8.device)
        pred = torch.empty((b, 2, 4, c), dtype=torch.float64, device=state_u8.device) if want_pred else None
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        self.tick_horizon_device(b, state_u8.data_ptr(), out.data_ptr(), dec.data_ptr(), pred.data_ptr() if want_pred else None,
                                 push.data_ptr() if push is not None else None, inst_u8.data_ptr() if inst_u8 is not None else None, stream)
        return out, dec, pred

    def rollout_device(self, batch, state_ptr, ticks, traj_ptr=None, stream=None):
        rc = _l().ismpc_a_rollout_device(self._h, int(batch), C.c_void_p(state_ptr), int(ticks),
                                         C.c_void_p(traj_ptr) if traj_ptr else None,
                                         C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    def rollout_mc_device(self, batch, state_ptr, ticks, inst_ptr=None, pushes_ptr=None, n_push=0, stride=1, traj_ptr=None,
                          summary_ptr=None, stream=None):
        """ismpc_a_rollout_mc_device on raw device pointers: the closed loop with per-instance velocity pushes (batch x n_push
        ismpc_a_push entries, instance-major), a trajectory row every `stride` ticks and one ismpc_a_rollout_summary per instance."""
        opt = lambda p: C.c_void_p(p) if p else None
        rc = _l().ismpc_a_rollout_mc_device(self._h, int(batch), opt(state_ptr), opt(inst_ptr), int(ticks), opt(pushes_ptr), int(n_push),
                                            int(stride), opt(traj_ptr), opt(summary_ptr), opt(stream))
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    def rollout_mc_torch(self, state_u8, ticks, pushes=None, stride=1, want_traj=True, want_summary=True, inst_u8=None):
        """The disturbed closed loop on torch tensors.  state_u8: CUDA uint8 [batch, 96], updated in place; pushes: None or a CUDA uint8
        tensor [batch, n_push, 24] of PUSH_A records; inst_u8: None (the handle's parameters) or CUDA uint8 [batch, 32] INST_A records.
        Returns (traj, summary): CUDA uint8 [ticks // stride, batch, 80] or None, and CUDA uint8 [batch, 64] (ROLLOUT_SUMMARY_A) or None."""
        import torch
        b = state_u8.shape[0]
        assert state_u8.is_cuda and state_u8.dtype == torch.uint8 and state_u8.shape[1] == 96 and state_u8.is_contiguous()
        n_push = 0
        if pushes is not None:
            assert pushes.is_cuda and pushes.dtype == torch.uint8 and pushes.dim() == 3 and pushes.shape[0] == b and pushes.shape[2] == 24 and pushes.is_contiguous()
            assert pushes.device == state_u8.device
            n_push = int(pushes.shape[1])
        if inst_u8 is not None:
            assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.shape == (b, 32) and inst_u8.is_contiguous()
        traj = torch.empty((ticks // stride if stride >= 1 else 0, b, 80), dtype=torch.uint8, device=state_u8.device) if want_traj else None
        summary = torch.empty((b, 64), dtype=torch.uint8, device=state_u8.device) if want_summary else None
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        self.rollout_mc_device(b, state_u8.data_ptr(), ticks, inst_u8.data_ptr() if inst_u8 is not None else None,
                               pushes.data_ptr() if n_push else None, n_push, stride,
                               traj.data_ptr() if want_traj else None, summary.data_ptr() if want_summary else None, stream)
        return traj, summary

    def rollout_mc_feet_device(self, batch, state_ptr, feet_ptr, ticks, inst_ptr=None, pushes_ptr=None, n_push=0, stride=1, traj_ptr=None,
                               summary_ptr=None, feet_summary_ptr=None, stream=None):
        """ismpc_a_rollout_mc_feet_device on raw device pointers: rollout_mc_device with the swing-foot QP of every instance behind every
        tick (feet_ptr: batch x feet_rows x 8 doubles, in place) and one ismpc_a_feet_summary per instance behind the last one."""
        opt = lambda p: C.c_void_p(p) if p else None
        rc = _l().ismpc_a_rollout_mc_feet_device(self._h, int(batch), opt(state_ptr), opt(inst_ptr), int(ticks), opt(pushes_ptr), int(n_push),
                                                 int(stride), opt(traj_ptr), opt(summary_ptr), opt(feet_ptr), opt(feet_summary_ptr), opt(stream))
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    def rollout_mc_feet_torch(self, state_u8, feet, ticks, pushes=None, stride=1, want_traj=True, want_summary=True, want_feet_summary=True,
                              inst_u8=None):
        """The disturbed closed loop with the swing-foot QPs on torch tensors.  state_u8, pushes, inst_u8: as rollout_mc_torch; feet: the
        CUDA float64 [batch, feet_rows, 8] block of feet_init_torch / feet_init_inst_torch, updated in place.  Returns (traj, summary,
        feet_summary): as rollout_mc_torch, and CUDA uint8 [batch, 32] (FEET_SUMMARY_A: the block as it stands against the base plan) or None."""
        import torch
        b = state_u8.shape[0]
        assert state_u8.is_cuda and state_u8.dtype == torch.uint8 and state_u8.shape[1] == 96 and state_u8.is_contiguous()
        n_push = 0
        if pushes is not None:
            assert pushes.is_cuda and pushes.dtype == torch.uint8 and pushes.dim() == 3 and pushes.shape[0] == b and pushes.shape[2] == 24 and pushes.is_contiguous()
            assert pushes.device == state_u8.device
            n_push = int(pushes.shape[1])
        if inst_u8 is not None:
            assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.shape == (b, 32) and inst_u8.is_contiguous()
        assert feet.is_cuda and feet.dtype == torch.float64 and feet.is_contiguous() and feet.device == state_u8.device
        assert tuple(feet.shape) == (b, _l().ismpc_a_feet_rows(self._h), 8)
        traj = torch.empty((ticks // stride if stride >= 1 else 0, b, 80), dtype=torch.uint8, device=state_u8.device) if want_traj else None
        summary = torch.empty((b, 64), dtype=torch.uint8, device=state_u8.device) if want_summary else None
        feet_summary = torch.empty((b, 32), dtype=torch.uint8, device=state_u8.device) if want_feet_summary else None
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        self.rollout_mc_feet_device(b, state_u8.data_ptr(), feet.data_ptr(), ticks, inst_u8.data_ptr() if inst_u8 is not None else None,
                                    pushes.data_ptr() if n_push else None, n_push, stride, traj.data_ptr() if want_traj else None,
                                    summary.data_ptr() if want_summary else None, feet_summary.data_ptr() if want_feet_summary else None, stream)
        return traj, summary, feet_summary

    def foot_trajectories_torch(self, feet, sim_duration, inst_u8=None):
        """The four foot files of every instance on the device (ismpc_a_foot_trajectories_device), bit for bit foot_trajectories() of the
        instance's rows of `feet` (CUDA float64 [batch, feet_rows, 8]).  inst_u8: None (the handle's step and plan 0) or CUDA uint8
        [batch, 32] INST_A records (step and base plan per instance).  Returns (files, nrows): CUDA float64 [batch, 4, sim_duration, 3] in
        the order fl, fr, rl, rr, and CUDA int32 [batch] with n_b = (sim_duration // step_b) * step_b, or -1 where foot_trajectories()
        would raise.  `files` is uninitialised memory: rows at and after nrows[b] (all rows where nrows[b] == -1) are unspecified."""
        import torch
        b = feet.shape[0]
        assert feet.is_cuda and feet.dtype == torch.float64 and feet.is_contiguous()
        assert tuple(feet.shape) == (b, _l().ismpc_a_feet_rows(self._h), 8)
        if inst_u8 is not None:
            assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.shape == (b, 32) and inst_u8.is_contiguous() and inst_u8.device == feet.device
        files = torch.empty((b, 4, max(int(sim_duration), 0), 3), dtype=torch.float64, device=feet.device)
        nrows = torch.empty((b,), dtype=torch.int32, device=feet.device)
        stream = torch.cuda.current_stream(feet.device).cuda_stream
        opt = lambda p: C.c_void_p(p) if p else None
        rc = _l().ismpc_a_foot_trajectories_device(self._h, b, opt(inst_u8.data_ptr() if inst_u8 is not None else None), opt(feet.data_ptr()),
                                                   int(sim_duration), opt(files.data_ptr()), opt(nrows.data_ptr()), opt(stream))
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return files, nrows

    def reserve(self, max_batch):
        """Sizes the handle's scratch for batches up to max_batch now (ismpc_a_reserve) instead of stream-ordered inside the calls."""
        if _l().ismpc_a_reserve(self._h, int(max_batch)) != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    def feet_init_torch(self, g, foot_plan, batch, device="cuda:0"):
        """Per-instance foot plans on the device: float64 tensor [batch, rows + FEET_PAD, 8]."""
        import torch
        fp = np.ascontiguousarray(foot_plan, dtype=np.float64)
        feet = torch.empty((batch, fp.shape[0] + FEET_PAD, 8), dtype=torch.float64, device=device)
        stream = torch.cuda.current_stream(feet.device).cuda_stream
        rc = _l().ismpc_a_feet_init_device(self._h, C.byref(g), fp.ctypes.data_as(C.c_void_p), fp.shape[0], int(batch),
                                           C.c_void_p(feet.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return feet

    def rollout_feet_torch(self, state_u8, feet, ticks):
        import torch
        b = state_u8.shape[0]
        traj = torch.empty((ticks, b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        rc = _l().ismpc_a_rollout_feet_device(self._h, b, C.c_void_p(state_u8.data_ptr()), int(ticks), C.c_void_p(traj.data_ptr()),
                                              C.c_void_p(feet.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return traj

    def last_deferred(self):
        """QPs the last fp32 launch handed to the fp64 re-solve launch behind it (synchronises)."""
        n = _l().ismpc_a_last_deferred(self._h)
        if n < 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return n

    def feet_init_inst_torch(self, gaits, foot_plans, inst_u8):
        """Per-instance gait parameters: one GaitA and one foot_plan per base plan of the handle (same row count); every
        instance starts from the foot plan of its own base plan.  Returns float64 tensor [batch, rows + FEET_PAD, 8]."""
        import torch
        rows = max(np.asarray(f).shape[0] for f in foot_plans)           # the trot generator writes n_gait rows, the walk one n_gait + 1:
        pad = lambda f: np.concatenate([f, np.repeat(f[-1:], rows - f.shape[0], 0)])   # a plan holds its last row beyond its end
        fps = np.ascontiguousarray(np.stack([pad(np.asarray(f, dtype=np.float64)) for f in foot_plans]))
        ga = (GaitA * len(gaits))(*gaits)
        b = inst_u8.shape[0]
        feet = torch.empty((b, fps.shape[1] + FEET_PAD, 8), dtype=torch.float64, device=inst_u8.device)
        stream = torch.cuda.current_stream(inst_u8.device).cuda_stream
        rc = _l().ismpc_a_feet_init_inst_device(self._h, C.cast(ga, C.c_void_p), fps.ctypes.data_as(C.c_void_p), fps.shape[1], len(gaits), b,
                                                C.c_void_p(inst_u8.data_ptr()), C.c_void_p(feet.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return feet

    def rollout_feet_inst_torch(self, state_u8, inst_u8, feet, ticks):
        import torch
        b = state_u8.shape[0]
        traj = torch.empty((ticks, b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        rc = _l().ismpc_a_rollout_feet_inst_device(self._h, b, C.c_void_p(state_u8.data_ptr()), C.c_void_p(inst_u8.data_ptr()), int(ticks),
                                                   C.c_void_p(traj.data_ptr()), C.c_void_p(feet.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return traj

    def tick_feet_torch(self, state_u8, feet, push=None):
        """One tick with the handle's parameters followed by the swing-foot QP of every instance (ismpc_a_tick_feet_batch_device).
        feet: the caller's float64 [batch, rows + FEET_PAD, 8] block, updated in place; push: None or CUDA float64 [batch, 2]."""
        import torch
        b = state_u8.shape[0]
        out = torch.empty((b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        rc = _l().ismpc_a_tick_feet_batch_device(self._h, b, C.c_void_p(state_u8.data_ptr()),
                                                 C.c_void_p(push.data_ptr()) if push is not None else None, C.c_void_p(out.data_ptr()),
                                                 C.c_void_p(feet.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return out

    def tick_feet_inst_torch(self, state_u8, inst_u8, feet, push=None):
        import torch
        b = state_u8.shape[0]
        out = torch.empty((b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        rc = _l().ismpc_a_tick_feet_batch_inst_device(self._h, b, C.c_void_p(state_u8.data_ptr()), C.c_void_p(inst_u8.data_ptr()),
                                                      C.c_void_p(push.data_ptr()) if push is not None else None, C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(feet.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return out

    def set_warm_history(self, enabled=True):
        """Caller-driven tick loops: start every QP from the working set the same instance had in the previous call."""
        if _l().ismpc_a_set_warm_history(self._h, 1 if enabled else 0) != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())

    # per-instance gait parameters (INST_A records): Monte-Carlo / sweep batches
    def add_plan(self, center):
        ce = np.ascontiguousarray(center, dtype=np.float64)
        if ce.shape != self.center.shape:
            raise ValueError("plan shape differs from the handle's")
        k = _l().ismpc_a_add_plan(self._h, ce.ctypes.data_as(C.c_void_p))
        if k < 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return k

    def tick_inst_torch(self, state_u8, inst_u8, push=None):
        import torch
        b = state_u8.shape[0]
        assert state_u8.is_cuda and state_u8.dtype == torch.uint8 and state_u8.shape[1] == 96 and state_u8.is_contiguous()
        assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.shape == (b, 32) and inst_u8.is_contiguous()
        out = torch.empty((b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        rc = _l().ismpc_a_tick_batch_inst_device(self._h, b, C.c_void_p(state_u8.data_ptr()), C.c_void_p(inst_u8.data_ptr()),
                                                 C.c_void_p(push.data_ptr()) if push is not None else None,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return out

    def rollout_inst_torch(self, state_u8, inst_u8, ticks):
        import torch
        b = state_u8.shape[0]
        assert inst_u8.is_cuda and inst_u8.dtype == torch.uint8 and inst_u8.shape == (b, 32) and inst_u8.is_contiguous()
        traj = torch.empty((ticks, b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        rc = _l().ismpc_a_rollout_inst_device(self._h, b, C.c_void_p(state_u8.data_ptr()), C.c_void_p(inst_u8.data_ptr()), int(ticks),
                                              C.c_void_p(traj.data_ptr()), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise IsmpcAError(_l().ismpc_a_last_error().decode())
        return traj

    # torch conveniences
    def tick_torch(self, state_u8, push=None):
        import torch
        b = state_u8.shape[0]
        assert state_u8.is_cuda and state_u8.dtype == torch.uint8 and state_u8.shape[1] == 96 and state_u8.is_contiguous()
        out = torch.empty((b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        self.tick_device(b, state_u8.data_ptr(), push.data_ptr() if push is not None else None, out.data_ptr(), stream)
        return out

    def rollout_torch(self, state_u8, ticks):
        import torch
        b = state_u8.shape[0]
        traj = torch.empty((ticks, b, 80), dtype=torch.uint8, device=state_u8.device)
        stream = torch.cuda.current_stream(state_u8.device).cuda_stream
        self.rollout_device(b, state_u8.data_ptr(), ticks, traj.data_ptr(), stream)
        return traj
