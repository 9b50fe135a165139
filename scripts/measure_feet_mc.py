#!/usr/bin/env python3
"""Numbers for DESIGN.md section 5, "Pushed closed loops with swing feet; foot files on the device" -- never the bench `value`.

  (a) what the swing-foot QPs cost inside the disturbed closed loop: rollout_mc_feet_torch against rollout_mc_torch on the same
      handle shape and inputs (walk configuration of BASELINE configs[3], 16 384 instances, 200 ticks, one push per instance at tick 0,
      rollout summary on, no trajectory), and the caller-driven tick_feet_torch loop users had before;
  (b) the expansion kernel (ismpc_a_foot_trajectories_device) at 16 384 instances x 2 000 rows: milliseconds and bytes written per
      second, next to a fill of the same buffer in the same process, and the host writer for 256 instances on one core scaled to the batch.

Every device figure is timed with events around one region, after warm-up regions, as the median [min - max] of --regions regions.
usage: python scripts/measure_feet_mc.py [--batch 16384] [--ticks 200] [--rows 2000] [--regions 20] [--leg walk_C150] [--precision f32] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import quadruped_gait_generation_ismpc_amd as q  # noqa: E402
from quadruped_gait_generation_ismpc_amd import workload, formulation_a as FA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--rows", type=int, default=2000)
ap.add_argument("--regions", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--leg", default="walk_C150")
ap.add_argument("--precision", default="f32")
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
assert args.regions >= 20 or args.batch < 16384, "at least 20 regions for a number that goes into DESIGN.md"
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def timed(region, reset):
    """Median [min, max] milliseconds of `region()` over args.regions regions, `reset()` before each one outside the events."""
    ms = []
    for k in range(args.warmup + args.regions):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); region(); e1.record(); e1.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), regions=len(ms))


B, T = args.batch, args.ticks
w = workload.make_batch_a(args.leg, B)
g = FA.default_gait(w["kind"], w["phi"], w["disp_A"])
fp, ce = FA.plan(g)
par = FA.default_params(w["kind"], C=w["C"], P=w["P"], F=w["F"])


def handle():
    gen = FA.GaitGenerator(par, ce, precision=args.precision)
    gen.reserve(B)
    return gen


d0 = q.to_device(w["state"]); d = d0.clone()
table = np.zeros((B, 1), dtype=FA.PUSH_A); table["dv"][:, 0] = w["push"]                  # one push per instance, at tick 0
d_table = q.to_device(table.reshape(-1)).view(B, 1, 24)
d_push = torch.zeros((T, B, 2), dtype=torch.float64, device="cuda:0"); d_push[0] = torch.from_numpy(w["push"].copy()).to("cuda:0")
base = dict(leg=args.leg, precision=args.precision, batch=B, ticks=T, device=torch.cuda.get_device_name(0))

# (a) the loop without feet, with feet, and driven by the caller
gen = handle()
r = timed(lambda: gen.rollout_mc_torch(d, T, pushes=d_table, want_traj=False), lambda: d.copy_(d0))
summ = q.from_device(gen.rollout_mc_torch(d.copy_(d0), T, pushes=d_table, want_traj=False)[1], FA.ROLLOUT_SUMMARY_A)
emit(dict(base, what="rollout_mc_torch", **r, us_per_tick=1e3 * r["ms_median"] / T, ticks_per_s=B * T / (1e-3 * r["ms_median"]),
          instances_with_error_ticks=int((summ["error_ticks"] > 0).sum())))
gen.close()

gen = handle()
feet0 = gen.feet_init_torch(g, fp, batch=B); feet = feet0.clone()


def reset_feet():
    d.copy_(d0); feet.copy_(feet0)


r = timed(lambda: gen.rollout_mc_feet_torch(d, feet, T, pushes=d_table, want_traj=False), reset_feet)
reset_feet()
fsum = q.from_device(gen.rollout_mc_feet_torch(d, feet, T, pushes=d_table, want_traj=False)[2], FA.FEET_SUMMARY_A)
emit(dict(base, what="rollout_mc_feet_torch", **r, us_per_tick=1e3 * r["ms_median"] / T, ticks_per_s=B * T / (1e-3 * r["ms_median"]),
          instances_with_moved_rows=int((fsum["moved_rows"] > 0).sum()), nonfinite=int(fsum["nonfinite"].sum())))
gen.close()

gen = handle()
gen.feet_init_torch(g, fp, batch=1)
gen.set_warm_history(True)


def caller_loop():
    for t in range(T):
        gen.tick_feet_torch(d, feet, d_push[t])


r = timed(caller_loop, reset_feet)
emit(dict(base, what="tick_feet_torch loop", **r, us_per_tick=1e3 * r["ms_median"] / T, ticks_per_s=B * T / (1e-3 * r["ms_median"])))

# (b) the four foot files of the batch on the device
S = args.rows
rows = FA._l().ismpc_a_feet_rows(gen._h)
n = (S // par.step) * par.step
dst = torch.empty((B, 4, S, 3), dtype=torch.float64, device="cuda:0")
nrows = torch.empty((B,), dtype=torch.int32, device="cuda:0")
stream = torch.cuda.current_stream().cuda_stream


def expand():
    rc = FA._l().ismpc_a_foot_trajectories_device(gen._h, B, None, C.c_void_p(feet.data_ptr()), S, C.c_void_p(dst.data_ptr()),
                                                  C.c_void_p(nrows.data_ptr()), C.c_void_p(stream) if stream else None)
    assert rc == 0, FA._l().ismpc_a_last_error().decode()


r = timed(expand, lambda: None)
written = B * 4 * n * 3 * 8
assert (nrows.cpu().numpy() == n).all()
emit(dict(batch=B, rows=S, what="ismpc_a_foot_trajectories_device", **r, bytes_written=written, bytes_read=B * rows * 64,
          TB_per_s_written=written / (1e-3 * r["ms_median"]) / 1e12, device=torch.cuda.get_device_name(0)))
r = timed(lambda: dst.fill_(1.0), lambda: None)
emit(dict(batch=B, rows=S, what="torch fill of the same buffer", **r, bytes_written=dst.numel() * 8,
          TB_per_s_written=dst.numel() * 8 / (1e-3 * r["ms_median"]) / 1e12))
expand(); torch.cuda.synchronize()
host_n = min(256, B)
fpl = feet[:host_n].cpu().numpy()
t0 = time.perf_counter()
host = [FA.foot_trajectories(g, par.step, fpl[b], S) for b in range(host_n)]
el = time.perf_counter() - t0
assert np.array_equal(dst[:host_n, :, :n].cpu().numpy(), np.stack(host)), "the device files are not the host writer's"
emit(dict(what="host ismpc_a_foot_trajectories, one core", instances=host_n, rows=S, ms=1e3 * el, ms_scaled_to_batch=1e3 * el * B / host_n,
          device_equals_host=True))
gen.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(lines, f, indent=1)
