"""Formulation A plan tables (ismpc_a_create_plans): the gait records the plan generators are checked on, and the oracle's generator
behind buffers that hold everything it writes; the 37-plan Monte-Carlo (records, reference-handle remapping, pushes) and the oracle's
closed loops in worker processes.  Shared by tests/test_plans_a_abi.py (host) and tests/test_gpu_plans_a.py (device)."""
import ctypes as C

import numpy as np

N_GAITS = (16, 23, 100)          # the smallest accepted value, one that ends inside the walk's eight-row pattern, the shipped value
# atan(0.8) is the clip's own threshold (disp_vertical / disp_forw = 0.4 / 0.5): one record on either side of it
PHIS = (0.0, np.pi / 4, np.pi / 2, np.arctan(0.8) + 1e-12, np.arctan(0.8) - 1e-12, -np.pi / 4)
DISP_AS = (0.05, 0.10, 0.15, 0.6)
N_RANDOM = 64


def grid_records(FA, kind, n_gait, seed=3):
    """The grid of headings and strides, then N_RANDOM random records (any heading, strides on both sides of the clips)."""
    recs = []
    for phi in PHIS:
        for dA in DISP_AS:
            g = FA.default_gait(kind, phi, dA); g.n_gait = n_gait
            recs.append(g)
    rng = np.random.default_rng(seed + 7 * kind + n_gait)
    for _ in range(N_RANDOM):
        g = FA.default_gait(kind, rng.uniform(-np.pi / 2, np.pi / 2), rng.uniform(0.02, 0.9)); g.n_gait = n_gait
        g.disp_B = rng.uniform(0.2, 0.3); g.disp_C = rng.uniform(0.7, 1.0)
        recs.append(g)
    return recs


def clip_branches(FA, recs):
    """OR of the clip branches (FA.CLIP_*) the records take."""
    seen = 0
    for g in recs:
        seen |= FA.plan_steps(g)[1]
    return seen


def oracle_plan(g):
    """oracle_a.plan(g) for any n_gait: the same orc_a_plan call behind buffers that hold every row it writes.  The walk generator
    writes whole eight-row patterns -- foot_plan rows up to n_gait + 7, centre rows up to n_gait + 2 -- and oracle_a.plan's own buffers
    (n_gait + 2 and n_gait + 1 rows) hold them for n_gait = 100 only.  Returns (foot_plan rows 1 .. used, center rows 1 .. n_gait)."""
    from oracle import oracle_a as A
    og = A.Gait(gait=g.gait, n_gait=g.n_gait, disp_A=g.disp_A, phi=g.phi, disp_B=g.disp_B, disp_C=g.disp_C, disp_i=g.disp_i,
                disp_o=g.disp_o, disp_forw=g.disp_forw)
    fp = np.zeros((g.n_gait + 16, 8)); ce = np.zeros((g.n_gait + 16, 2))
    used = A._lib().orc_a_plan(C.byref(og), fp.ctypes.data_as(C.c_void_p), ce.ctypes.data_as(C.c_void_p))
    return fp[1:used + 1].copy(), ce[1:g.n_gait + 1].copy()


# ---- the 37-plan Monte-Carlo of tests/test_gpu_plans_a.py: the reference's own ranges of heading and stride
N37, PER_PLAN = 37, 4
PHI37 = np.linspace(0.0, np.pi / 2, N37)
DISP_A37 = np.where(np.arange(N37) % 2 == 0, 0.10, 0.15)
LOOP_TICKS, LOOP_STRIDE, LOOP_SAMPLE = 120, 3, 16
# seed of the instance draw, the pushes and the oracle sample of the closed loops: the first one tried; the oracle alone, without pushes,
# stays feasible (status 0 on every tick) on all LOOP_SAMPLE sampled instances (test_closed_loops_against_the_oracle asserts it)
LOOP_SEED = 5


def gaits37(FA, shape):
    """shape "walk" / "trot": 37 records of that gait; "mc": trot on even plans, walk on odd ones."""
    kind = lambda k: {"walk": FA.WALK, "trot": FA.TROT}.get(shape, FA.TROT if k % 2 == 0 else FA.WALK)
    return [FA.default_gait(kind(k), float(PHI37[k]), float(DISP_A37[k])) for k in range(N37)]


def params37(FA, shape):
    if shape == "mc":
        return FA.default_params(FA.TROT, C=200, P=400, F=6)
    return FA.default_params(FA.WALK if shape == "walk" else FA.TROT)


def instances37(FA, shape, gaits, seed=LOOP_SEED, per_plan=PER_PLAN):
    """per_plan instances per plan in shuffled order.  "mc": the draw of _mc_instances (test_gpu_formulation_a.py; BASELINE configs[4]) --
    height ~ U(0.50, 0.62), step ~ U{40..100}, ds = round(0.6 step), F = ceil(C / step) + 1, Qf by the plan's gait; else the handle's own
    parameters in every record."""
    rng = np.random.default_rng(seed)
    par = params37(FA, shape)
    n = len(gaits) * per_plan
    inst = np.zeros(n, dtype=FA.INST_A)
    plan = rng.permutation(np.repeat(np.arange(len(gaits)), per_plan))
    for i in range(n):
        trot = gaits[plan[i]].gait == FA.TROT
        if shape == "mc":
            step = int(rng.integers(40, 101))
            inst[i] = (rng.uniform(0.50, 0.62), 1e7 if trot else 1e9, step, int(round(0.6 * step)), -(-par.C // step) + 1, plan[i])
        else:
            inst[i] = (par.height, par.Qf, par.step, par.ds, par.F, plan[i])
    return inst


def initial_states(FA, gaits, centers, inst):
    """quad_walk_no_plots.m:52-62 per instance, from the HOST's plan of its gait record."""
    st = np.zeros(len(inst), dtype=FA.STATE_A)
    for i, k in enumerate(inst["plan"]):
        st["x"][i] = st["xz"][i] = gaits[k].disp_C / 2
        st["cur_x"][i], st["cur_y"][i] = centers[k][0]
    st["fc"] = 1; st["j"] = 1
    return st


def group_of(plan):
    return plan // 4


def remap(inst, g):
    """The records as reference handle g (plans 4 g .. 4 g + 3 of the table, registered by ismpc_a_create + ismpc_a_add_plan) takes them:
    the plan index inside the group, 0 for the instances of other groups.  Returns (records, mask of the group's own instances)."""
    own = group_of(inst["plan"]) == g
    r = inst.copy()
    r["plan"] = np.where(own, inst["plan"] - 4 * g, 0)
    return r, own


def two_pushes(FA, n, ticks, seed=LOOP_SEED):
    """Two pushes per instance at two different ticks in [5, ticks - 5), ascending, of the bench's size (0.03, 0.05 m/s)."""
    rng = np.random.default_rng(seed + 1000)
    t = np.zeros((n, 2), dtype=FA.PUSH_A)
    for i in range(n):
        t["tick"][i] = np.sort(rng.choice(np.arange(5, ticks - 5), 2, replace=False))
    t["dv"][..., 0] = rng.uniform(-0.03, 0.03, (n, 2)); t["dv"][..., 1] = rng.uniform(-0.05, 0.05, (n, 2))
    return t


def loop_sample(n, seed=LOOP_SEED):
    return np.sort(np.random.default_rng(seed + 2000).choice(n, LOOP_SAMPLE, replace=False))


def oracle_loop(g, par, rec, ticks, pushes=None):
    """One oracle on the instance's own plan (gait record g) and parameters (INST_A record rec over the handle's par): `ticks` closed-loop
    ticks, pushes (PUSH_A entries, ascending ticks) applied as the device applies them.  Returns the TICK_A records [ticks]."""
    from oracle import oracle_a as A
    p = A.params(g.gait, C_=par.C, P=par.P, F=int(rec["F"]), step=int(rec["step"]), ds=int(rec["ds"]), Qf=float(rec["Qf"]), n_gait=g.n_gait)
    p.height = float(rec["height"])
    sim = A.SimA(A.gait(g.gait, g.phi, g.disp_A, n_gait=g.n_gait), p, backend="gi")
    at = {} if pushes is None else {int(e["tick"]): tuple(e["dv"]) for e in pushes}
    return np.array([sim.tick(at.get(t, (0.0, 0.0))) for t in range(ticks)], dtype=A.TICK_A)


def oracle_loops(FA, jobs, nproc=16):
    """oracle_loop for every (gait record, params, INST_A record, ticks, pushes or None) of `jobs`, in worker PROCESSES that never touch
    the GPU (a closed loop of 120 ticks at C = 200 takes the oracle about two seconds; the calling test process holds the GPU and must
    not fork: tests/helpers/oracle_a_pool.py is the precedent).  Returns the TICK_A arrays in the order of `jobs`."""
    import os, pickle, subprocess, sys, tempfile
    from oracle import oracle_a as A
    fields = lambda s: {k: getattr(s, k) for k, _ in s._fields_}
    items = [dict(g=fields(g), par=fields(par), rec=rec.tobytes(), ticks=ticks, pushes=None if pushes is None else pushes.tobytes())
             for g, par, rec, ticks, pushes in jobs]
    nproc = max(1, min(nproc, os.cpu_count() or 1, len(items)))
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with tempfile.TemporaryDirectory() as td:
        procs = []
        for k in range(nproc):
            with open(os.path.join(td, f"in{k}.pkl"), "wb") as f:
                pickle.dump(items[k::nproc], f)
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), os.path.join(td, f"in{k}.pkl"), os.path.join(td, f"out{k}.pkl")],
                                          cwd=root, stderr=subprocess.PIPE, text=True))
        out = [None] * len(items)
        for k, pr in enumerate(procs):
            _, err = pr.communicate(timeout=600)
            if pr.returncode != 0:
                raise RuntimeError("oracle worker failed: " + (err or "")[-800:])
            with open(os.path.join(td, f"out{k}.pkl"), "rb") as f:
                for j, r in enumerate(pickle.load(f)):
                    out[k + j * nproc] = np.frombuffer(r, dtype=A.TICK_A).copy()
    return out


def _worker(src, dst):
    import os, pickle, sys
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA       # the record types; loads no native code
    with open(src, "rb") as f:
        items = pickle.load(f)
    res = []
    for it in items:
        g = FA.GaitA(**it["g"]); par = FA.ParamsA(**it["par"])
        rec = np.frombuffer(it["rec"], dtype=FA.INST_A)[0]
        pushes = None if it["pushes"] is None else np.frombuffer(it["pushes"], dtype=FA.PUSH_A)
        res.append(oracle_loop(g, par, rec, it["ticks"], pushes).tobytes())
    with open(dst, "wb") as f:
        pickle.dump(res, f)


def assert_plan_is_the_oracles(got_fp, got_ce, g):
    """(foot_plan, center) as the product returns them against the oracle, to the bit.  The product caps the foot plan at n_gait + 1 rows
    (ismpc_a.h); the scripts' array grows to the end of the last eight-row pattern."""
    ofp, oce = oracle_plan(g)
    rows = g.n_gait if g.gait == 0 else min(ofp.shape[0], g.n_gait + 1)
    assert got_fp.shape == (rows, 8), (got_fp.shape, rows)
    assert ofp.shape[0] >= rows
    assert np.array_equal(got_fp, ofp[:rows]), (g.gait, g.n_gait, g.phi, g.disp_A)
    assert got_ce.shape == oce.shape and np.array_equal(got_ce, oce), (g.gait, g.n_gait, g.phi, g.disp_A)


if __name__ == "__main__":
    import sys
    _worker(sys.argv[1], sys.argv[2])
