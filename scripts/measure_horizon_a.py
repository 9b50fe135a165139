#!/usr/bin/env python3
"""Numbers for DESIGN.md section 5, "The whole decision and the predicted horizon of a tick" -- never the bench `value`.

What ismpc_a_tick_batch_horizon_device costs over the plain tick, at the two Formulation A bench shapes (BASELINE configs[3]: walk,
C = 150, 16 384 instances; configs[4]: Monte-Carlo, C = 200, per-instance gait parameters, 16 384 instances), in fp64 and fp32:
milliseconds per tick of
    plain      tick_torch / tick_inst_torch (the bench's own timed call)
    dec        the horizon tick with pred_dev = NULL: the solver kernels' decision stores, 2 (C + F) doubles per instance
    dec+pred   ... and ismpc_a_predict_kernel behind them, 8 C doubles per instance more
on the same inputs: the bench leg's state and push, restored before every region outside the events.  Output buffers are allocated once.
Every figure is timed with events around one region, after warm-up regions, as the median [min - max] of --regions regions; the three
forms are interleaved region by region so that clock and thermal drift fall on all of them alike.
usage: python scripts/measure_horizon_a.py [--batch 16384] [--regions 30] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import quadruped_gait_generation_ismpc_amd as q  # noqa: E402
from quadruped_gait_generation_ismpc_amd import workload, formulation_a as FA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--regions", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--preroll", type=int, default=60)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
B = args.batch
lines = []


def emit(rec):
    lines.append(rec)
    print(json.dumps(rec), flush=True)


def setup(leg, precision):
    """(gen, state0, push, inst or None) of a bench leg."""
    if leg == "mc_C200":
        inst, push = workload.make_inst_mc(B)
        plans = [FA.plan(FA.default_gait(k, np.pi / 4, 0.1))[1] for k in (0, 1)]
        par = FA.default_params(0, C=200, P=400, F=6)
        gen = FA.GaitGenerator(par, plans[0], precision=precision); gen.add_plan(plans[1])
        d_inst = q.to_device(inst)
        d0 = q.to_device(gen.initial_state(0.88, batch=B))
        prep = FA.GaitGenerator(par, plans[0]); prep.add_plan(plans[1])
        prep.rollout_inst_torch(d0, d_inst, args.preroll); torch.cuda.synchronize(); prep.close()      # spreads the gait phases, as bench.py does
        return gen, d0, torch.from_numpy(push.copy()).to("cuda:0"), d_inst
    w = workload.make_batch_a(leg, B)
    g = FA.default_gait(w["kind"], w["phi"], w["disp_A"])
    gen = FA.GaitGenerator(FA.default_params(w["kind"], C=w["C"], P=w["P"], F=w["F"]), FA.plan(g)[1], precision=precision)
    return gen, q.to_device(w["state"]), torch.from_numpy(w["push"].copy()).to("cuda:0"), None


for leg in ("walk_C150", "mc_C200"):
    for precision in ("f64", "f32"):
        gen, d0, push, inst = setup(leg, precision)
        gen.reserve(B)
        C_, F_ = gen.horizon_shape()
        d = d0.clone()
        out = torch.empty((B, 80), dtype=torch.uint8, device="cuda:0")
        dec = torch.empty((B, 2, C_ + F_), dtype=torch.float64, device="cuda:0")
        pred = torch.empty((B, 2, 4, C_), dtype=torch.float64, device="cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        ip = inst.data_ptr() if inst is not None else None
        forms = {
            "plain": (lambda: gen.tick_inst_torch(d, inst, push)) if inst is not None else (lambda: gen.tick_torch(d, push)),
            "dec": lambda: gen.tick_horizon_device(B, d.data_ptr(), out.data_ptr(), dec.data_ptr(), None, push.data_ptr(), ip, stream),
            "dec+pred": lambda: gen.tick_horizon_device(B, d.data_ptr(), out.data_ptr(), dec.data_ptr(), pred.data_ptr(), push.data_ptr(), ip, stream),
        }
        ms = {k: [] for k in forms}
        for r in range(args.warmup + args.regions):
            for k, fn in forms.items():
                d.copy_(d0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                if r >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        base = float(np.median(ms["plain"]))
        for k, v in ms.items():
            v = np.array(v)
            emit(dict(leg=leg, precision=precision, batch=B, C=C_, F=F_, what=k, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()),
                      regions=len(v), us_over_plain=1e3 * (float(np.median(v)) - base),
                      bytes_out=(0 if k == "plain" else dec.numel() * 8 + (pred.numel() * 8 if k == "dec+pred" else 0)), device=torch.cuda.get_device_name(0)))
        gen.close()
if args.out:
    with open(args.out, "w") as f:
        json.dump(lines, f, indent=1)
