"""Multi-GPU groups over the C ABI of include/ismpc_group.h: a batch of independent gait instances cut into contiguous
shards, one per GPU, and the path's one collective -- the all-gather of the 80-byte output records -- issued by the native
library on RCCL.  Nothing here computes or communicates in Python; torch only lends device memory.

    Group(plan, params, devices=[0, 1, ...])                      one process drives n devices   (ismpc_group_create)
    Group.from_rank(plan, params, device, uid, rank, world)       one process per GPU             (ismpc_group_create_rank)
    uid = unique_id()  on rank 0, distributed by the caller (bench.py: torch.distributed over gloo)
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import TICK_IN, TICK_OUT, PUSH, ROLLOUT_SUMMARY

EXPORTS_GROUP = ["ismpc_shard_range", "ismpc_group_unique_id", "ismpc_group_create", "ismpc_group_create_rank", "ismpc_group_destroy",
                 "ismpc_group_world", "ismpc_group_local", "ismpc_group_rank", "ismpc_group_handle", "ismpc_group_solve_batch",
                 "ismpc_group_step_device", "ismpc_group_result_device", "ismpc_group_wait_on", "ismpc_group_sync", "ismpc_group_reserve", "ismpc_group_order_after",
                 "ismpc_a_group_create", "ismpc_a_group_create_rank", "ismpc_a_group_destroy", "ismpc_a_group_world", "ismpc_a_group_local",
                 "ismpc_a_group_rank", "ismpc_a_group_handle", "ismpc_a_group_add_plan", "ismpc_a_group_set_precision", "ismpc_a_group_tick_batch",
                 "ismpc_a_group_step_device", "ismpc_a_group_result_device", "ismpc_a_group_wait_on", "ismpc_a_group_sync", "ismpc_a_group_reserve", "ismpc_a_group_order_after",
                 "ismpc_group_rollout_mc_device", "ismpc_group_rollout_wait_on", "ismpc_group_reserve_rollout",
                 "ismpc_a_group_rollout_mc_device", "ismpc_a_group_rollout_wait_on", "ismpc_a_group_reserve_rollout",
                 "ismpc_records_to_instance_major_device",
                 "ismpc_group_last_error", "ismpc_group_rccl_version"]
UNIQUE_ID_BYTES = 128
_bound = False


class GroupError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ismpc group error {code}: {msg}")
        self.code = code


def _l():
    global _bound
    lib = _lib.load()
    if not _bound:
        vp, ci = C.c_void_p, C.c_int
        pi = C.POINTER(C.c_int)
        lib.ismpc_shard_range.argtypes = [ci, ci, ci, pi, pi]; lib.ismpc_shard_range.restype = ci
        lib.ismpc_group_unique_id.argtypes = [vp]; lib.ismpc_group_unique_id.restype = ci
        lib.ismpc_group_create.argtypes = [vp, vp, ci, pi, ci, C.POINTER(vp)]; lib.ismpc_group_create.restype = ci
        lib.ismpc_group_create_rank.argtypes = [vp, vp, ci, ci, vp, ci, ci, C.POINTER(vp)]; lib.ismpc_group_create_rank.restype = ci
        lib.ismpc_a_group_create.argtypes = [vp, vp, pi, ci, C.POINTER(vp)]; lib.ismpc_a_group_create.restype = ci
        lib.ismpc_a_group_create_rank.argtypes = [vp, vp, ci, vp, ci, ci, C.POINTER(vp)]; lib.ismpc_a_group_create_rank.restype = ci
        for pre in ("ismpc_group_", "ismpc_a_group_"):
            getattr(lib, pre + "destroy").argtypes = [vp]; getattr(lib, pre + "destroy").restype = None
            for f in ("world", "local", "sync"):
                getattr(lib, pre + f).argtypes = [vp]; getattr(lib, pre + f).restype = ci
            getattr(lib, pre + "rank").argtypes = [vp, ci]; getattr(lib, pre + "rank").restype = ci
            getattr(lib, pre + "handle").argtypes = [vp, ci]; getattr(lib, pre + "handle").restype = vp
            getattr(lib, pre + "result_device").argtypes = [vp, ci, ci, C.POINTER(vp)]; getattr(lib, pre + "result_device").restype = ci
            getattr(lib, pre + "wait_on").argtypes = [vp, ci, ci, vp]; getattr(lib, pre + "wait_on").restype = ci
            getattr(lib, pre + "order_after").argtypes = [vp, ci, vp]; getattr(lib, pre + "order_after").restype = ci
            getattr(lib, pre + "reserve").argtypes = [vp, ci]; getattr(lib, pre + "reserve").restype = ci
            getattr(lib, pre + "rollout_wait_on").argtypes = [vp, ci, vp]; getattr(lib, pre + "rollout_wait_on").restype = ci
            getattr(lib, pre + "reserve_rollout").argtypes = [vp, ci, ci]; getattr(lib, pre + "reserve_rollout").restype = ci
        lib.ismpc_group_solve_batch.argtypes = [vp, ci, vp, vp]; lib.ismpc_group_solve_batch.restype = ci
        lib.ismpc_group_step_device.argtypes = [vp, ci, C.POINTER(vp), ci]; lib.ismpc_group_step_device.restype = ci
        lib.ismpc_a_group_add_plan.argtypes = [vp, vp]; lib.ismpc_a_group_add_plan.restype = ci
        lib.ismpc_a_group_set_precision.argtypes = [vp, ci]; lib.ismpc_a_group_set_precision.restype = ci
        lib.ismpc_a_group_tick_batch.argtypes = [vp, ci, vp, vp, vp, vp]; lib.ismpc_a_group_tick_batch.restype = ci
        lib.ismpc_a_group_step_device.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), ci]; lib.ismpc_a_group_step_device.restype = ci
        pv = C.POINTER(vp)
        lib.ismpc_group_rollout_mc_device.argtypes = [vp, ci, pv, ci, ci, pv, ci, ci, pv, pv]; lib.ismpc_group_rollout_mc_device.restype = ci
        lib.ismpc_a_group_rollout_mc_device.argtypes = [vp, ci, pv, pv, ci, pv, ci, ci, pv, pv]; lib.ismpc_a_group_rollout_mc_device.restype = ci
        lib.ismpc_records_to_instance_major_device.argtypes = [vp, ci, ci, vp, vp]; lib.ismpc_records_to_instance_major_device.restype = ci
        lib.ismpc_group_last_error.argtypes = []; lib.ismpc_group_last_error.restype = C.c_char_p
        lib.ismpc_group_rccl_version.argtypes = []; lib.ismpc_group_rccl_version.restype = ci
        _bound = True
    return lib


def _check(rc):
    if rc < 0:
        raise GroupError(rc, _l().ismpc_group_last_error().decode())
    return rc


def shard_range(batch, rank, world):
    """ismpc_shard_range: contiguous shard [first, first + count) of `rank`; the first batch % world ranks hold one more."""
    f, c = C.c_int(), C.c_int()
    _check(_l().ismpc_shard_range(int(batch), int(rank), int(world), C.byref(f), C.byref(c)))
    return f.value, c.value


def unique_id():
    """128 opaque bytes naming a new RCCL communicator (rank 0 makes them, every rank of the group passes the same bytes)."""
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    _check(_l().ismpc_group_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


def rccl_version():
    return int(_l().ismpc_group_rccl_version())


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*[C.c_void_p(int(p)) if p else None for p in ptrs])


def records_to_instance_major(tick_major_u8, out=None):
    """ismpc_records_to_instance_major_device on torch tensors: CUDA uint8 [rows, count, 80] (a rollout's trajectory) -> [count, rows, 80], on the
    current stream of the tensor's device.  `out`: a contiguous CUDA uint8 [count, rows, 80] (a shard's block of a larger buffer), else allocated."""
    import torch
    src = tick_major_u8
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3 and src.shape[2] == 80 and src.is_contiguous()
    rows, count = int(src.shape[0]), int(src.shape[1])
    if out is None:
        out = torch.empty((count, rows, 80), dtype=torch.uint8, device=src.device)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (count, rows, 80) and out.is_contiguous() and out.device == src.device
    with torch.cuda.device(src.device):
        _check(_l().ismpc_records_to_instance_major_device(C.c_void_p(src.data_ptr()), rows, count, C.c_void_p(out.data_ptr()),
                                                           C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)))
    return out


class _DeviceBytes:
    """Device memory owned by the native library, described to torch through the CUDA array interface."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


class _GroupBase:
    _pre = "ismpc_group_"

    def _f(self, name):
        return getattr(self._lib, self._pre + name)

    @property
    def world(self):
        """Ranks of the communicator as RCCL itself reports them (ncclCommCount)."""
        return _check(self._f("world")(self._g))

    @property
    def n_local(self):
        return _check(self._f("local")(self._g))

    def rank(self, local=0):
        return _check(self._f("rank")(self._g, int(local)))

    def shard(self, batch, local=0):
        return shard_range(batch, self.rank(local), self.world)

    def reserve(self, max_batch):
        _check(self._f("reserve")(self._g, int(max_batch)))

    def sync(self):
        _check(self._f("sync")(self._g))

    def wait_on(self, local, buf, stream):
        _check(self._f("wait_on")(self._g, int(local), int(buf), C.c_void_p(int(stream)) if stream else None))

    def order_after(self, local, stream):
        """The group's launch stream of local device `local` waits for what is enqueued so far on the caller's stream."""
        _check(self._f("order_after")(self._g, int(local), C.c_void_p(int(stream)) if stream else None))

    def rollout_wait_on(self, local, stream):
        """The caller's stream waits for the most recent rollout of local device `local`: its collective, and so its kernels too."""
        _check(self._f("rollout_wait_on")(self._g, int(local), C.c_void_p(int(stream)) if stream else None))

    def reserve_rollout(self, max_batch, max_rows):
        """Sizes the group's tick-major trajectory buffer and the handles' scratch for rollouts up to max_batch x max_rows now."""
        _check(self._f("reserve_rollout")(self._g, int(max_batch), int(max_rows)))

    def _rollout_mc_host(self, state, rec_bytes, pushes, push_dtype, summary_dtype, rows, want_traj, want_summary, inst, call):
        """numpy in, numpy out around rollout_mc_device of a ONE-PROCESS group: torch lends the memory of every local device, every device's
        shard of the states comes back, the gathered outputs are read from local device 0."""
        import torch
        from .solver import to_device, from_device
        batch = state.shape[0]
        n_push = 0
        if pushes is not None:
            pushes = np.ascontiguousarray(pushes, dtype=push_dtype).reshape(batch, -1)
            n_push = pushes.shape[1]
        if inst is not None:
            assert inst.shape == (batch,)
        out_state = state.copy()
        empty_traj = np.zeros((batch, 0), dtype=rec_bytes) if want_traj and rows == 0 else None      # zero rows: no trajectory buffer is passed
        want_traj = want_traj and rows > 0
        if batch == 0:
            return out_state, (np.zeros((0, rows), dtype=rec_bytes) if want_traj else empty_traj), (np.zeros(0, dtype=summary_dtype) if want_summary else None)
        st, pu, ins, tr, su = [], [], [], [], []
        for l, d in enumerate(self.devices):
            dev = torch.device("cuda", d)
            first, count = self.shard(batch, l)
            st.append(to_device(state[first:first + count], dev) if count else None)
            pu.append(to_device(pushes[first:first + count], dev) if count and n_push else None)
            ins.append(to_device(inst[first:first + count], dev) if count and inst is not None else None)
            tr.append(torch.empty((batch * rows, 80), dtype=torch.uint8, device=dev) if want_traj else None)
            su.append(torch.empty((batch, summary_dtype.itemsize), dtype=torch.uint8, device=dev) if want_summary else None)
            self.order_after(l, torch.cuda.current_stream(dev).cuda_stream)
        ptrs = lambda ts: [t.data_ptr() if t is not None else None for t in ts]
        call(batch, ptrs(st), ptrs(ins) if inst is not None else None, ptrs(pu) if n_push else None, n_push,
             ptrs(tr) if want_traj else None, ptrs(su) if want_summary else None)
        self.sync()
        for l in range(len(self.devices)):
            first, count = self.shard(batch, l)
            if count:
                out_state[first:first + count] = from_device(st[l], state.dtype)
        traj = from_device(tr[0], rec_bytes).reshape(batch, rows) if want_traj else empty_traj
        return out_state, traj, (from_device(su[0], summary_dtype) if want_summary else None)

    def result_ptr(self, local, buf):
        p = C.c_void_p()
        _check(self._f("result_device")(self._g, int(local), int(buf), C.byref(p)))
        return p.value

    def result_torch(self, batch, local=0, buf=0):
        """The gathered buffer of local device `local` as a uint8 tensor [batch, 80]: a zero-copy VIEW of the group's memory (valid until the
        step after next overwrites the buffer).  The current stream of that device is made to wait for the collective first."""
        import torch
        dev = torch.device("cuda", self.devices[local])
        self.wait_on(local, buf, torch.cuda.current_stream(dev).cuda_stream)
        view = _DeviceBytes(self.result_ptr(local, buf), int(batch) * 80)
        return torch.as_tensor(view, device=dev).view(int(batch), 80)

    def close(self):
        if getattr(self, "_g", None):
            self._f("destroy")(self._g); self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group(_GroupBase):
    """Formulation B (MPCSolver::solve) on several GPUs: ismpc_group_*."""

    def __init__(self, ftsp_and_timings, params, devices=(0,), _rank=None):
        self._lib = _l()
        self.params = params
        self.ftsp = np.ascontiguousarray(ftsp_and_timings, dtype=np.float64)
        if self.ftsp.ndim != 2 or self.ftsp.shape[1] != 4:
            raise ValueError("ftsp_and_timings must be rows x 4")
        g = C.c_void_p()
        if _rank is None:
            self.devices = [int(d) for d in devices]
            arr = (C.c_int * len(self.devices))(*self.devices)
            _check(self._lib.ismpc_group_create(C.cast(C.byref(params), C.c_void_p), self.ftsp.ctypes.data_as(C.c_void_p), self.ftsp.shape[0],
                                                arr, len(self.devices), C.byref(g)))
        else:
            device, uid, rank, world = _rank
            if len(uid) != UNIQUE_ID_BYTES:
                raise ValueError("the unique id is 128 bytes")
            self.devices = [int(device)]
            ub = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(uid)
            _check(self._lib.ismpc_group_create_rank(C.cast(C.byref(params), C.c_void_p), self.ftsp.ctypes.data_as(C.c_void_p), self.ftsp.shape[0],
                                                     int(device), C.cast(ub, C.c_void_p), int(rank), int(world), C.byref(g)))
        self._g = g

    @classmethod
    def from_rank(cls, ftsp_and_timings, params, device, uid, rank, world):
        return cls(ftsp_and_timings, params, _rank=(device, uid, rank, world))

    def solve_batch(self, tick_in, out=None):
        """Host records in, ALL host records out (ismpc_group_solve_batch)."""
        tick_in = np.ascontiguousarray(tick_in, dtype=TICK_IN).reshape(-1)
        if out is None:
            out = np.zeros(tick_in.shape[0], dtype=TICK_OUT)
        assert out.dtype == TICK_OUT and out.flags.c_contiguous and out.shape == tick_in.shape
        _check(self._lib.ismpc_group_solve_batch(self._g, tick_in.shape[0], tick_in.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def step_device(self, batch, shard_ptrs, buf):
        """One asynchronous step: shard_ptrs[l] = device pointer of local device l's shard of ismpc_tick_in records."""
        _check(self._lib.ismpc_group_step_device(self._g, int(batch), _ptr_array(shard_ptrs), int(buf)))


    def rollout_mc_device(self, batch, state_ptrs, first_frame, ticks, pushes_ptrs=None, n_push=0, stride=1, traj_all_ptrs=None, summary_all_ptrs=None):
        """ismpc_group_rollout_mc_device, asynchronous: lists of device pointers, one per local device -- the shard's states (advanced in place) and
        push tables, and the caller's gathered buffers: batch x (ticks // stride) records, instance-major, and batch summaries (None: not wanted)."""
        opt = lambda ps: _ptr_array(ps) if ps is not None else None
        _check(self._lib.ismpc_group_rollout_mc_device(self._g, int(batch), opt(state_ptrs), int(first_frame), int(ticks), opt(pushes_ptrs), int(n_push),
                                                       int(stride), opt(traj_all_ptrs), opt(summary_all_ptrs)))

    def rollout_mc(self, state, first_frame, ticks, pushes=None, stride=1, want_traj=True, want_summary=True):
        """The disturbed closed loop of a one-process group on host records: state TICK_IN [batch], pushes None or PUSH [batch, n_push].  Returns
        (final_state, traj, summary): TICK_IN [batch], TICK_OUT [batch, ticks // stride] or None, ROLLOUT_SUMMARY [batch] or None."""
        state = np.ascontiguousarray(state, dtype=TICK_IN).reshape(-1)
        call = lambda b, st, ins, pu, n_push, tr, su: self.rollout_mc_device(b, st, first_frame, ticks, pu, n_push, stride, tr, su)
        return self._rollout_mc_host(state, TICK_OUT, pushes, PUSH, ROLLOUT_SUMMARY, int(ticks) // int(stride), want_traj, want_summary, None, call)


class GroupA(_GroupBase):
    """Formulation A (the MATLAB generators' tick) on several GPUs: ismpc_a_group_*."""
    _pre = "ismpc_a_group_"

    def __init__(self, params, center, devices=(0,), _rank=None):
        self._lib = _l()
        self.params = params
        self.center = np.ascontiguousarray(center, dtype=np.float64)
        g = C.c_void_p()
        if _rank is None:
            self.devices = [int(d) for d in devices]
            arr = (C.c_int * len(self.devices))(*self.devices)
            _check(self._lib.ismpc_a_group_create(C.cast(C.byref(params), C.c_void_p), self.center.ctypes.data_as(C.c_void_p), arr, len(self.devices), C.byref(g)))
        else:
            device, uid, rank, world = _rank
            self.devices = [int(device)]
            ub = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(uid)
            _check(self._lib.ismpc_a_group_create_rank(C.cast(C.byref(params), C.c_void_p), self.center.ctypes.data_as(C.c_void_p), int(device),
                                                       C.cast(ub, C.c_void_p), int(rank), int(world), C.byref(g)))
        self._g = g

    @classmethod
    def from_rank(cls, params, center, device, uid, rank, world):
        return cls(params, center, _rank=(device, uid, rank, world))

    def add_plan(self, center):
        c = np.ascontiguousarray(center, dtype=np.float64)
        return _check(self._lib.ismpc_a_group_add_plan(self._g, c.ctypes.data_as(C.c_void_p)))

    def set_precision(self, fp32):
        _check(self._lib.ismpc_a_group_set_precision(self._g, 1 if fp32 else 0))

    def tick_batch(self, state, inst=None, push=None):
        """Host records: `state` (STATE_A, updated in place for this process's shards), optional per-instance records and pushes; returns all
        output records (ismpc_a_group_tick_batch)."""
        from .formulation_a import STATE_A, OUT_A, INST_A
        assert state.dtype == STATE_A and state.flags.c_contiguous
        n = state.shape[0]
        out = np.zeros(n, dtype=OUT_A)
        ip = None
        if inst is not None:
            inst = np.ascontiguousarray(inst, dtype=INST_A); assert inst.shape == (n,)
            ip = inst.ctypes.data_as(C.c_void_p)
        pp = None
        if push is not None:
            push = np.ascontiguousarray(push, dtype=np.float64); assert push.shape == (n, 2)
            pp = push.ctypes.data_as(C.c_void_p)
        _check(self._lib.ismpc_a_group_tick_batch(self._g, n, state.ctypes.data_as(C.c_void_p), ip, pp, out.ctypes.data_as(C.c_void_p)))
        return out

    def step_device(self, batch, state_ptrs, inst_ptrs, push_ptrs, buf):
        _check(self._lib.ismpc_a_group_step_device(self._g, int(batch), _ptr_array(state_ptrs), _ptr_array(inst_ptrs) if inst_ptrs else None,
                                                   _ptr_array(push_ptrs) if push_ptrs else None, int(buf)))

    def rollout_mc_device(self, batch, state_ptrs, ticks, inst_ptrs=None, pushes_ptrs=None, n_push=0, stride=1, traj_all_ptrs=None, summary_all_ptrs=None):
        """ismpc_a_group_rollout_mc_device, asynchronous: lists of device pointers, one per local device (as Group.rollout_mc_device; inst_ptrs: None or
        the shards' per-instance records)."""
        opt = lambda ps: _ptr_array(ps) if ps is not None else None
        _check(self._lib.ismpc_a_group_rollout_mc_device(self._g, int(batch), opt(state_ptrs), opt(inst_ptrs), int(ticks), opt(pushes_ptrs), int(n_push),
                                                         int(stride), opt(traj_all_ptrs), opt(summary_all_ptrs)))

    def rollout_mc(self, state, ticks, pushes=None, stride=1, want_traj=True, want_summary=True, inst=None):
        """The disturbed closed loop of a one-process group on host records: state STATE_A [batch], pushes None or PUSH_A [batch, n_push], inst None or
        INST_A [batch].  Returns (final_state, traj, summary): STATE_A [batch], OUT_A [batch, ticks // stride] or None, ROLLOUT_SUMMARY_A [batch] or None."""
        from .formulation_a import STATE_A, OUT_A, INST_A, PUSH_A, ROLLOUT_SUMMARY_A
        state = np.ascontiguousarray(state, dtype=STATE_A).reshape(-1)
        if inst is not None:
            inst = np.ascontiguousarray(inst, dtype=INST_A).reshape(-1)
        call = lambda b, st, ins, pu, n_push, tr, su: self.rollout_mc_device(b, st, ticks, ins, pu, n_push, stride, tr, su)
        return self._rollout_mc_host(state, OUT_A, pushes, PUSH_A, ROLLOUT_SUMMARY_A, int(ticks) // int(stride), want_traj, want_summary, inst, call)
