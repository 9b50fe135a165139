#!/usr/bin/env python3
"""Disturbed closed-loop rollouts through a group of ONE device (real RCCL), Formulation B, beside bench.py:
  plain   ismpc_rollout_mc_device on a plain handle (works with any build of the library: ISMPC_LIB=<an older one> for an A/B)
  group   the group call end to end (order_after -> rollout -> rollout_wait_on on the caller's stream), one call and two back to back
  pack    the record transposition kernel alone against hipMemcpyAsync device-to-device of the same bytes, same process
Each figure: device events around every repetition; median, min and max of the repetitions are printed as one JSON line.
usage: python scripts/group_rollout_probe.py plain|group|pack [batch [ticks [reps]]]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import quadruped_gait_generation_ismpc_amd as q  # noqa: E402

mode = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
T = int(sys.argv[3]) if len(sys.argv) > 3 else 200
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 20
STRIDES = (1, 10)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "reps": len(a)}


def timed(body, before=None, reps=REPS, warm=3):
    """body() enqueues on the current stream; before() restores the inputs outside the timed window."""
    out = []
    for k in range(warm + reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); body(); e1.record(); e1.synchronize()
        if k >= warm:
            out.append(e0.elapsed_time(e1))
    return out


def inputs():
    st0 = np.repeat(np.zeros(1, dtype=q.TICK_IN), B); st0["com_pos"][:, 2] = 0.69
    rng = np.random.default_rng(1)
    st0["com_pos"][:, :2] += rng.uniform(-0.004, 0.004, (B, 2)); st0["com_vel"][:, :2] += rng.uniform(-0.02, 0.02, (B, 2))
    pu = np.zeros((B, 2), dtype=q.PUSH)
    pu["tick"][:, 0] = rng.integers(0, max(T // 2, 1), B); pu["tick"][:, 1] = pu["tick"][:, 0] + rng.integers(1, max(T // 2, 2), B)
    pu["dv"][:, :, :2] = rng.uniform(-0.03, 0.03, (B, 2, 2))
    return q.to_device(st0), q.to_device(pu.reshape(-1))


p = q.default_params(N=100)
plan = q.reference_plan(params=p)
d_st0, d_pu = inputs()
d_st = d_st0.clone()
stream = torch.cuda.current_stream().cuda_stream
base = {"mode": mode, "batch": B, "ticks": T, "lib": os.environ.get("ISMPC_LIB", "in-tree")}

if mode == "plain":
    s = q.MPCSolver(plan, params=p, device=0)
    s.reserve(B)
    d_sm = torch.empty((B, 48), dtype=torch.uint8, device="cuda:0")
    for stride in STRIDES:
        d_tr = torch.empty((T // stride, B, 80), dtype=torch.uint8, device="cuda:0")
        ms = timed(lambda: s.rollout_mc_device(B, d_st.data_ptr(), 0, T, d_pu.data_ptr(), 2, stride, d_tr.data_ptr(), d_sm.data_ptr(), stream),
                   before=lambda: d_st.copy_(d_st0))
        r = dict(base, what="ismpc_rollout_mc_device", stride=stride, **stats(ms)); r["ticks_per_s"] = B * T / (1e-3 * r["median_ms"])
        print(json.dumps(r), flush=True)
        del d_tr
    s.close()
elif mode == "group":
    from quadruped_gait_generation_ismpc_amd import group as G
    g = G.Group(plan, p, devices=[0])
    d_st2 = d_st0.clone()
    d_sm = torch.empty((B, 48), dtype=torch.uint8, device="cuda:0")
    for stride in STRIDES:
        rows = T // stride
        g.reserve_rollout(B, rows)
        d_tr = torch.empty((B * rows, 80), dtype=torch.uint8, device="cuda:0")

        def call(state):
            g.rollout_mc_device(B, [state.data_ptr()], 0, T, [d_pu.data_ptr()], 2, stride, [d_tr.data_ptr()], [d_sm.data_ptr()])

        def one():
            g.order_after(0, stream); call(d_st); g.rollout_wait_on(0, stream)

        def two():
            g.order_after(0, stream); call(d_st); call(d_st2); g.rollout_wait_on(0, stream)

        def restore():
            d_st.copy_(d_st0); d_st2.copy_(d_st0)
        a, b = stats(timed(one, before=restore)), stats(timed(two, before=restore))
        print(json.dumps(dict(base, what="group call, end to end", stride=stride, rows=rows, **a)), flush=True)
        print(json.dumps(dict(base, what="two group calls back to back", stride=stride, rows=rows, **b,
                              reuse_wait_ms=b["median_ms"] - 2 * a["median_ms"])), flush=True)
        g.sync()
        del d_tr
    g.close()
elif mode == "pack":
    from quadruped_gait_generation_ismpc_amd import group as G
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]; hip.hipMemcpyAsync.restype = C.c_int
    for stride in STRIDES:
        rows = T // stride
        src = torch.randint(0, 256, (rows, B, 80), dtype=torch.uint8, device="cuda:0")
        dst = torch.empty((B, rows, 80), dtype=torch.uint8, device="cuda:0")
        nbytes = src.numel()
        k = stats(timed(lambda: G.records_to_instance_major(src, out=dst)))
        assert torch.equal(dst, src.permute(1, 0, 2))

        def copy():
            assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, stream) == 0          # 3 = hipMemcpyDeviceToDevice
        c = stats(timed(copy))
        tb = lambda s_: 2 * nbytes / (1e-3 * s_["median_ms"]) / 1e12                                  # read + written, TB/s
        print(json.dumps(dict(base, what="records_to_instance_major", stride=stride, rows=rows, bytes_moved=2 * nbytes, **k, TB_per_s=tb(k))), flush=True)
        print(json.dumps(dict(base, what="hipMemcpyAsync device to device", stride=stride, rows=rows, bytes_moved=2 * nbytes, **c, TB_per_s=tb(c))), flush=True)
        del src, dst
else:
    raise SystemExit(__doc__)
