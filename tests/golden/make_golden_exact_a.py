#!/usr/bin/env python3
"""Generates tests/golden/formA_exact_<group>.npz: Formulation A ticks solved in exact arithmetic (tests/helpers/exact_tick_a.py, mpmath),
rounded to fp64 once, with their certificates, margins and working sets, and the FLOOR of every group per quantity.  A kernel tolerance
is derived from that floor and from nothing else (tests/test_gpu_exact_parity_a.py: 16 x in fp64, 16 x 2^29 x in fp32).

A tick is kept only when both QPs certify with a slack margin >= 1e-8 m and a multiplier margin >= 1e-6 of the largest multiplier, five
orders above the fp64 kernels' violation threshold: a kernel that ends on another working set is wrong, not unlucky.  At most 10 % of the
drawn single ticks of a group may be dropped on margin grounds; a closed loop is kept whole (or redrawn by hand with another push).
Drawn and kept counts are stored.

The floor is the larger of two reference-side errors against the exact values, neither of them the code under test:
  floor_oracle   the fp64 oracle ("gi": a dense Goldfarb-Idnani on the same QP) -- single ticks through load_product_state, loops as the
                 oracle's own loop;
  floor_numpy    a plain numpy fp64 solve of the certified working set's KKT system, on the oracle's fp64 QP data, with the LIP update
                 and the bookkeeping in numpy -- single ticks from the fixture's state, loops as a closed loop of its own.
In both, cur / off is taken as at least the f0 error (exact_tick_a.reference_floor: cur is f0 on a switching tick, the input otherwise).

Every state comes from a nominal closed loop of the oracle (the product's record is the oracle's state plus the plan shift
off = f0 - center[fc] of the last footstep switch and the `rebuilt` flag); pushes are drawn as tests/test_gpu_formulation_a_edges.py draws
them.  Timing rule, phi and disp_A are that file's.

Run on the CPU:  python tests/golden/make_golden_exact_a.py [group ...]      (minutes; needs mpmath and the built oracle)
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle_a as A  # noqa: E402
from helpers import exact_tick_a as X  # noqa: E402

PHI, DISP_A = np.pi / 4, 0.1
MAX_BYTES = 100_000
KINDS = {"trot": A.TROT, "walk": A.WALK}
EDGES = (("walk", 5, 3), ("walk", 65, 4), ("trot", 129, 5), ("walk", 193, 6), ("walk", 250, 6), ("trot", 253, 3))
STATE_KEYS = ("x", "xd", "xz", "y", "yd", "yz", "cur_x", "cur_y")


def timing(kind_name, C, F):
    step, ds = (50, 30) if kind_name == "walk" else (80, 50)
    if -(-C // step) + 1 > F:
        step = max(4, -(-C // (F - 1))); ds = int(round(0.6 * step))
    return step, ds


def draw_pushes(seed, n):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.03, 0.03, n), rng.uniform(-0.05, 0.05, n)], 1)


def centers():
    """The two base plans, [2, n_gait, 2]: index 0 trot, 1 walk (the order the per-instance handles register them)."""
    return np.stack([A.plan(A.gait(k, PHI, DISP_A))[1] for k in (A.TROT, A.WALK)])


CENTERS = None


def make_sim(kind, par, backend="gi"):
    p = A.params(kind, C_=par.C, P=par.P, F=par.F, step=par.step, ds=par.ds, Qf=par.Qf)
    p.height = par.height
    return A.SimA(A.gait(kind, PHI, DISP_A), p, backend=backend)


def plain_par(kind_name, C, F):
    step, ds = timing(kind_name, C, F)
    return X.Par(A.params(KINDS[kind_name], C_=C, P=2 * C, F=F, step=step, ds=ds))


def product_state(st, off, rebuilt):
    rec = np.zeros(1, X.STATE_A)
    for k in STATE_KEYS + ("fc", "j"):
        rec[k] = st[k]
    rec["off_x"], rec["off_y"], rec["rebuilt"] = off[0], off[1], rebuilt
    return rec[0]


def nominal_states(kind, par, ticks, pushes=None, backend="gi"):
    """The product-format state before every tick 0 .. ticks of the oracle's own closed loop (pushes: {tick: (px, py)}), and its records."""
    sim = make_sim(kind, par, backend)
    center = CENTERS[kind]
    off, rebuilt = np.zeros(2), 0
    states, recs = [product_state(sim.state, off, rebuilt)], []
    for t in range(ticks):
        r = sim.tick(tuple((pushes or {}).get(t, (0.0, 0.0))))
        assert r["rv"][0] == 0 and r["rv"][1] == 0, (t, r["rv"])
        if r["stepped"]:
            off, rebuilt = r["f0"] - center[int(r["fc"])], 1           # off = f0 - center[new fc - 1], as the kernels form it
        recs.append(r.copy())
        states.append(product_state(sim.state, off, rebuilt))
    return states, recs


def oracle_tick(sim, center, rec, push):
    """(OUT_A, STATE_A after, (sol_x, sol_y), rv) of the fp64 oracle from one product state."""
    sim.load_product_state(rec)
    r, sx, sy = sim.tick(tuple(push), want_solution=True)
    off = np.array([rec["off_x"], rec["off_y"]]); rebuilt = int(rec["rebuilt"])
    if r["stepped"]:
        off, rebuilt = r["f0"] - center[int(r["fc"])], 1
    o = np.zeros(1, X.OUT_A)
    for k in ("com_before", "vel_after", "u0", "f0"):
        o[k][0] = r[k]
    return o[0], product_state(sim.state, off, rebuilt), (sx, sy), r["rv"].copy()


def numpy_tick(sim, center, par, rec, push, t):
    """A plain numpy fp64 solve of the certified working sets' KKT systems on the oracle's fp64 QP data, LIP update and bookkeeping in numpy."""
    pushed = rec.copy()
    pushed["xd"] = np.float64(rec["xd"]) + np.float64(push[0]); pushed["yd"] = np.float64(rec["yd"]) + np.float64(push[1])
    sim.load_product_state(pushed)
    C, F, dt = par.C, par.F, par.dt
    o, s = np.zeros(1, X.OUT_A), np.zeros(1, X.STATE_A)
    eta = np.sqrt(par.grav / par.height)
    ch, sh = np.cosh(eta * dt), np.sinh(eta * dt)
    Au = np.array([[ch, sh / eta, 1 - ch], [eta * sh, ch, -eta * sh], [0, 0, 1]]); Bu = np.array([dt - sh / eta, 1 - ch, dt])
    stepped = int(rec["j"]) + 1 >= par.step * int(rec["fc"])
    for ax in (0, 1):
        q = sim.axis_data(ax)
        W = t.axes[ax]["W"]
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
        rhs = np.concatenate([np.zeros(C), par.Qf * q["pref"], d])
        z = np.linalg.solve(K, rhs)
        u0, f0 = z[0], z[C]
        x = np.array([pushed["xy"[ax]], pushed[("xd", "yd")[ax]], pushed[("xz", "yz")[ax]]])
        nx = Au @ x + Bu * u0
        o["com_before"][0, ax], o["vel_after"][0, ax], o["u0"][0, ax], o["f0"][0, ax] = x[0], nx[1], u0, f0
        for k, v in zip(("xy"[ax], ("xd", "yd")[ax], ("xz", "yz")[ax]), nx):
            s[k][0] = v
        cur, off = ("cur_x", "cur_y")[ax], ("off_x", "off_y")[ax]
        s[cur][0], s[off][0] = (f0, f0 - center[int(rec["fc"]), ax]) if stepped else (rec[cur], rec[off])
    s["fc"][0], s["j"][0], s["rebuilt"][0] = int(rec["fc"]) + int(stepped), int(rec["j"]) + 1, 1 if stepped else int(rec["rebuilt"])
    return o[0], s[0]


class Group:
    def __init__(self, name, loop=False):
        self.name, self.loop = name, loop
        self.pars, self.case, self.plan, self.state, self.push, self.inst, self.rows = [], [], [], [], [], [], []
        self.outs, self.afters, self.ticks = [], [], []
        self.orc, self.npy = [], []
        self.drawn = 0
        self.sims = {}

    def case_of(self, par):
        key = tuple(par.row())
        for k, p in enumerate(self.pars):
            if tuple(p.row()) == key:
                return k
        self.pars.append(par)
        return len(self.pars) - 1

    def sim(self, kind, par):
        key = (kind,) + tuple(par.row())
        if key not in self.sims:
            self.sims[key] = make_sim(kind, par)
        return self.sims[key]

    def try_add(self, kind, handle_par, rec, push, inst=None):
        """Solve one tick exactly; keep it when both QPs certify with the margins.  handle_par: the handle's parameters (inst overrides)."""
        self.drawn += 1
        par = X.Par(handle_par, inst)
        center = CENTERS[kind]
        sim = self.sim(kind, par)
        o_orc, s_orc, hint, rv = oracle_tick(sim, center, rec, push)
        if rv.any():
            return None
        t = X.exact_tick_a(handle_par, center, rec, push, inst, hint)
        if not X.kept(t):
            print(f"  {self.name}: C {par.C} F {par.F} j {int(rec['j'])} dropped (certified {t.ok}, margins {[[float(v) for v in m] for m in getattr(t, 'margins', [])]})")
            return None
        o, s = X.to_records(t)
        self.case.append(self.case_of(X.Par(handle_par))); self.plan.append(kind); self.state.append(rec.copy()); self.push.append(np.array(push, float))
        ir = np.zeros(1, X.INST_A)
        if inst is not None:
            ir[0] = inst
        self.inst.append(ir[0]); self.outs.append(o); self.afters.append(s); self.ticks.append(t)
        self.orc.append((o_orc, s_orc)); self.npy.append(numpy_tick(sim, center, par, rec, push, t))
        return t, s

    def __len__(self):
        return len(self.ticks)

    def save(self, has_inst=False, loop_oracle=None):
        n = len(self)
        width = max(t.p.C + t.p.F for t in self.ticks)
        exact = X.quantities(np.array(self.outs), np.array(self.afters))
        orc = loop_oracle if loop_oracle is not None else X.quantities(np.array([o for o, _ in self.orc]), np.array([s for _, s in self.orc]))
        npy = X.quantities(np.array([o for o, _ in self.npy]), np.array([s for _, s in self.npy]))
        for other in (orc, npy):
            for k in X.COUNTERS:
                assert np.array_equal(other[k], exact[k]), (self.name, k)
        f_orc, f_npy = X.reference_floor(X.errors(orc, exact)), X.reference_floor(X.errors(npy, exact))
        floor = np.array([max(f_orc[k], f_npy[k]) for k in X.QUANTITIES])
        rows = [X.tick_arrays(t, width) for t in self.ticks]
        sol_idx = np.arange(0, n, 4 if self.loop else 2, dtype=np.int32)      # whole solutions and multipliers: of these ticks only (file size)
        data = dict(params=np.stack([p.row() for p in self.pars]), case=np.array(self.case, np.int32), centers=CENTERS, plan=np.array(self.plan, np.int32),
                    state=np.array(self.state).view(np.uint8).reshape(n, -1), push=np.stack(self.push), inst=np.array(self.inst).view(np.uint8).reshape(n, -1),
                    has_inst=np.int32(has_inst), loop=np.int32(self.loop), out=np.array(self.outs).view(np.uint8).reshape(n, -1),
                    state_after=np.array(self.afters).view(np.uint8).reshape(n, -1), ws=np.stack([r["ws"] for r in rows]),
                    margins=np.stack([r["margins"] for r in rows]), sol_idx=sol_idx, sol=np.stack([rows[i]["sol"] for i in sol_idx]),
                    mu=np.stack([rows[i]["mu"] for i in sol_idx]), floor=floor, floor_oracle=np.array([f_orc[k] for k in X.QUANTITIES]),
                    floor_numpy=np.array([f_npy[k] for k in X.QUANTITIES]),
                    drawn=np.int32(self.drawn), kept=np.int32(n))
        path = os.path.join(HERE, f"formA_exact_{self.name}.npz")
        np.savez_compressed(path, **data)
        size = os.path.getsize(path)
        act = X.active_sizes(np.array(self.outs))
        print(f"{self.name}: kept {n} of {self.drawn}, {size} bytes, working sets {act.min()}..{act.max()} (median {int(np.median(act))}), "
              f"margins slack {data['margins'][:, :, 0].min():.2e} mult {data['margins'][:, :, 1].min():.2e}")
        for nm, f in (("floor", floor), ("oracle", data["floor_oracle"]), ("numpy", data["floor_numpy"])):
            print(f"  {nm:7s}" + " ".join(f"{k}={v:.2e}" for k, v in zip(X.QUANTITIES, f)))
        assert n >= 0.9 * self.drawn, (self.name, n, self.drawn)
        assert size <= MAX_BYTES, (self.name, size)


def spread_ticks(step):
    """16 ticks of a nominal loop: spread, on both sides of the first two footstep switches (tick step - 2 runs with j = step - 1 and
    switches; before it rebuilt = 0), so rebuilt is 0 on six and 1 on ten."""
    return [0, 5, step // 3, step - 3, step - 2, step - 1, step, step + 1, step + step // 2, 2 * step - 3, 2 * step - 2, 2 * step - 1,
            2 * step, 2 * step + 7, 2 * step + step // 2, 3 * step - 2]


def single_ticks(g, kind_name, C, F, ticks, seed):
    par = plain_par(kind_name, C, F)
    kind = KINDS[kind_name]
    states, _ = nominal_states(kind, par, max(ticks))
    for t, push in zip(ticks, draw_pushes(seed, len(ticks))):
        g.try_add(kind, par, states[t], push)


def group_plain(name, kind_name, C, seed):
    g = Group(name)
    single_ticks(g, kind_name, C, 3, spread_ticks(timing(kind_name, C, 3)[0]), seed)
    return g


def group_edges():
    g = Group("edges")
    for k, (kind_name, C, F) in enumerate(EDGES):
        step = timing(kind_name, C, F)[0]
        single_ticks(g, kind_name, C, F, [0, step // 4, step // 2, step - 2, step - 1, step + 6], 20 + k)
    return g


def inst_draw(n=16, C=200, seed=5):
    """Per-instance records in the style of the Monte-Carlo draw of tests/test_gpu_formulation_a.py (_mc_instances): trot / walk by parity,
    height ~ U(0.50, 0.62), step ~ U{40..100}, ds = round(0.6 step), F = ceil(C / step) + 1 -- which gives F = 3 .. 6 at C = 200; the
    last two take step = C, the only timing with F = 2."""
    rng = np.random.default_rng(seed)
    inst = np.zeros(n, X.INST_A)
    for i in range(n):
        trot = i % 2 == 0
        step = int(rng.integers(40, 101)) if i < n - 2 else C
        inst[i] = (rng.uniform(0.50, 0.62), 1e7 if trot else 1e9, step, int(round(0.6 * step)), -(-C // step) + 1, 0 if trot else 1)
    return inst


def group_inst():
    g = Group("inst_C200")
    C = 200
    handle = X.Par(A.params(A.TROT, C_=C, P=2 * C, F=6))
    inst = inst_draw()
    assert set(inst["F"].tolist()) == {2, 3, 4, 5, 6}, sorted(set(inst["F"].tolist()))
    pushes = draw_pushes(2, len(inst))
    for i, rec in enumerate(inst):
        kind = int(rec["plan"])
        # a quarter of the instances on the tick that switches to the second footstep (j = step - 1: cur = f0, off = f0 - center of the
        # instance's own plan, rebuilt 0 -> 1), a quarter on the switch to the third (rebuilt already 1), trot and walk plans in both
        t = int(rec["step"]) - 2 if i % 8 in (0, 1) else 2 * int(rec["step"]) - 2 if i % 8 in (4, 5) else (13 * i) % 120
        states, _ = nominal_states(kind, X.Par(handle, rec), t)
        g.try_add(kind, handle, states[t], pushes[i], rec)
    return g


def group_loop(name, kind_name, C, F, pushes):
    """One closed loop of step + 12 ticks: the exact tick applied tick by tick, its state rounded to fp64 at every tick (the state record
    is fp64 by the ABI: what a kernel is given at tick k + 1 is what it stored at tick k), hints from the oracle at the exact loop's own
    states.  Kept whole."""
    g = Group(name, loop=True)
    par = plain_par(kind_name, C, F)
    kind = KINDS[kind_name]
    ticks = par.step + 12
    states, recs = nominal_states(kind, par, ticks, pushes)
    rec = states[0]
    for t in range(ticks):
        res = g.try_add(kind, par, rec, pushes.get(t, (0.0, 0.0)))
        assert res is not None, (name, t, "the loop is kept whole: redraw the push")
        rec = res[1]
    # the numpy side of the floor as a closed loop of its own too (the certified working sets of the exact loop: the two states differ by
    # rounding, the margins are 1e-8): an error of u0 at one tick is in the CoM of every later one, amplified by the LIP's unstable mode
    sim, rec, g.npy = g.sim(kind, par), states[0], []
    for t in range(ticks):
        g.npy.append(numpy_tick(sim, CENTERS[kind], par, rec, pushes.get(t, (0.0, 0.0)), g.ticks[t]))
        rec = g.npy[-1][1]
    o = np.zeros(ticks, X.OUT_A)
    for k in ("com_before", "vel_after", "u0", "f0"):
        o[k] = np.array([r[k] for r in recs])
    return g, X.quantities(o, np.array(states[1:]))


GROUPS = ("walk_C100", "trot_C160", "edges", "inst_C200", "loop_walk_C100", "loop_trot_C65")
LOOP_PUSHES = {"loop_walk_C100": {17: (0.021, -0.034), 53: (-0.017, 0.029)}, "loop_trot_C65": {30: (0.019, -0.027)}}


def build_group(name):
    global CENTERS
    if CENTERS is None:
        CENTERS = centers()
    if name == "walk_C100":
        return group_plain(name, "walk", 100, 11), {}
    if name == "trot_C160":
        return group_plain(name, "trot", 160, 12), {}
    if name == "edges":
        return group_edges(), {}
    if name == "inst_C200":
        return group_inst(), dict(has_inst=True)
    if name == "loop_walk_C100":
        g, own = group_loop(name, "walk", 100, 3, LOOP_PUSHES[name])
        return g, dict(loop_oracle=own)
    if name == "loop_trot_C65":
        g, own = group_loop(name, "trot", 65, 3, LOOP_PUSHES[name])
        return g, dict(loop_oracle=own)
    raise KeyError(name)


def main():
    for name in (sys.argv[1:] or GROUPS):
        t0 = time.time()
        g, kw = build_group(name)
        g.save(**kw)
        print(f"  ({time.time() - t0:.0f} s)")


if __name__ == "__main__":
    main()
