#!/usr/bin/env python3
"""Generates tests/golden/formA_horizon_floors.npz: per group of tests/golden/formA_exact_*.npz the FLOORS the whole decision and the
predicted horizon of a tick are held to (tests/test_gpu_horizon_a.py: 16 x in fp64, 16 x 2^29 x in fp32), over the group's sol_idx ticks
and both axes.  A floor is reference-side arithmetic, never the code under test:

  floor_u, floor_f   the larger of two errors against the fixture's exact whole solution `sol` (u = sol[:C], f = sol[C:C+F]):
                       the fp64 oracle's whole solution (load_product_state + tick(want_solution=True) on the fixture's state and push);
                       a plain numpy KKT solve of the certified working set `ws` on the oracle's fp64 QP data, the whole z kept
                       (make_golden_exact_a.numpy_tick keeps z[0] and z[C] of the same solve).
  floor_pred[4]      per row x, xd, xz, zc: horizon_a.predict_numpy against horizon_a.predict_exact, both fed the exact decision rounded
                     to fp64 and the oracle's next state as sample 1.

Run on the CPU:  python tests/golden/make_golden_horizon_a.py      (about a minute; needs mpmath and the built oracle)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden_exact_a as G  # noqa: E402
from helpers import exact_tick_a as X  # noqa: E402
from helpers import horizon_a as H  # noqa: E402

MAX_BYTES = 100_000
PATH = os.path.join(HERE, "formA_horizon_floors.npz")


def numpy_kkt(sim, par, rec, push, ws):
    """[2, C + F]: the whole z of a plain fp64 solve of the KKT system of the working sets ws[ax, row - 1] = sign."""
    pushed = rec.copy()
    pushed["xd"] = np.float64(rec["xd"]) + np.float64(push[0]); pushed["yd"] = np.float64(rec["yd"]) + np.float64(push[1])
    sim.load_product_state(pushed)
    C, F, dt = par.C, par.F, par.dt
    sol = np.zeros((2, C + F))
    for ax in (0, 1):
        q = sim.axis_data(ax)
        W = [(i + 1, int(s)) for i, s in enumerate(ws[ax, :C + F]) if s != 0]
        Aw = np.zeros((1 + len(W), C + F)); d = np.zeros(1 + len(W))
        Aw[0, :C] = q["a"]; d[0] = q["b"]
        for n, (i, sg) in enumerate(W, 1):
            if i <= C:
                Aw[n, :i] = dt; Aw[n, C:] = -q["M"][i - 1, 1:]; d[n] = q["zhi"][i - 1] if sg > 0 else q["zlo"][i - 1]
            else:
                r = i - C
                Aw[n, C + r - 1] = 1.0
                if r >= 2:
                    Aw[n, C + r - 2] = -1.0
                d[n] = q["khi"][r - 1] if sg > 0 else q["klo"][r - 1]
        h = np.concatenate([np.ones(C), np.full(F, par.Qf)])
        K = np.zeros((C + F + len(d), C + F + len(d)))
        K[:C + F, :C + F] = np.diag(h); K[:C + F, C + F:] = Aw.T; K[C + F:, :C + F] = Aw
        sol[ax] = np.linalg.solve(K, np.concatenate([np.zeros(C), par.Qf * q["pref"], d]))[:C + F]
    return sol


def group_floors(name):
    fx = X.load_group(name)
    states = fx["state"].view(X.STATE_A).reshape(-1)
    insts = fx["inst"].view(X.INST_A).reshape(-1)
    fu = ff = 0.0
    fp = np.zeros(4)
    sims = {}
    for n, idx in enumerate(fx["sol_idx"]):
        kind = int(fx["plan"][idx])
        par = X.Par(fx["params"][fx["case"][idx]], insts[idx] if fx["has_inst"] else None)
        key = (kind,) + tuple(par.row())
        if key not in sims:
            sims[key] = G.make_sim(kind, par)
        sim, rec, push = sims[key], states[idx], fx["push"][idx]
        C, F = par.C, par.F
        exact = fx["sol"][n][:, :C + F]
        _, s_orc, (sx, sy), rv = G.oracle_tick(sim, G.CENTERS[kind], rec, push)
        assert not rv.any(), (name, idx)
        for got in (np.stack([sx, sy]), numpy_kkt(sim, par, rec, push, fx["ws"][idx])):
            fu = max(fu, float(np.abs(got[:, :C] - exact[:, :C]).max()))
            ff = max(ff, float(np.abs(got[:, C:] - exact[:, C:]).max()))
        first = H.first_of(s_orc)
        e = np.abs(H.predict_numpy(par, rec, push, exact, first) - H.predict_exact(par, rec, push, exact, first))
        fp = np.maximum(fp, e.max(axis=(0, 2)))
    return fu, ff, fp


def main():
    G.CENTERS = G.centers()
    data = {}
    for name in G.GROUPS:
        fu, ff, fp = group_floors(name)
        data[f"{name}_floor_u"], data[f"{name}_floor_f"], data[f"{name}_floor_pred"] = np.float64(fu), np.float64(ff), fp
        print(f"{name}: floor_u {fu:.3e} floor_f {ff:.3e} floor_pred " + " ".join(f"{k}={v:.3e}" for k, v in zip(H.ROWS, fp)))
    np.savez_compressed(PATH, **data)
    size = os.path.getsize(PATH)
    print(f"{PATH}: {size} bytes")
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
