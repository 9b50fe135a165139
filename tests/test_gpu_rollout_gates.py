"""GPU tests of the closed loops (ismpc_rollout_device, ismpc_rollout_mc_device) at ticks that do NOT run: gated ticks
(mpc_dt = 2 control_dt: every second tick is ISMPC_ST_TICK_SKIPPED), the end of the footstep plan inside a rollout (ISMPC_ST_BAD_INDEX
from there on), the NaN guard (ISMPC_ST_Z_NAN) fed back by the loop, and a vertical solve that fails on every tick (ISMPC_ST_Z_FAILED:
flagged, never fed back).  The in-kernel loop carries the state in registers, the one-launch-per-tick loop goes through memory, the
resume launch mixes both: the three are compared byte for byte with each other and with a loop the test drives itself around
ismpc_solve_batch (the caller's bookkeeping restated in numpy), and every one of them with the CPU oracle's rollout.

The scenarios, and everything that is asserted about them from the oracle alone, are in tests/helpers/rollout_gate_cases.py (and are
checked without a GPU by tests/test_rollout_gate_cases.py).  Measured maxima go to stdout ("gates[...]") and into docs/dispatch_parity.md.
"""
import numpy as np
import pytest

from helpers import rollout_gate_cases as G
from test_gpu_rollout_mc import (q, O, TOL, make_under, run_mc, run_plain, segmented, reduce_summary,      # noqa: F401  (q, O: fixtures)
                                 assert_summary_equal)

pytestmark = pytest.mark.gpu

B = G.B
LANES = (8, 16, 32)
VEL_TOL = 1e-6                   # absolute, on the velocity (the issue's bound)
COUNTERS = ("control_iter", "mpc_iter", "footstep_counter", "simulation_time")


class Handles:
    """Creates handles under exactly the given knobs and closes every one of them when the block ends."""

    def __init__(self, q):
        self.q, self.made = q, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.made:
            s.close()

    def plain(self, env, params, plan):
        s = make_under(env, lambda: self.q.MPCSolver(plan, params=params))
        self.made.append(s)
        return s

    def sweep(self, env, sets, plan):
        s = make_under(env, lambda: self.q.MPCSolver.sweep(plan, sets))
        self.made.append(s)
        return s


def layout(lanes, host=False):
    env = {"ISMPC_PATH": "affine", "ISMPC_LPI": str(lanes)}
    if host:
        env["ISMPC_ROLLOUT"] = "host"
    return env


def device_params(q, name, **over):
    sc = G.SCENARIOS[name]
    return q.default_params(N=sc["N"], mpc_dt=sc["mpc_dt"], **over)


def family_of(s):
    info = s.launch_info()
    return f"{info['family']}/{info['lanes']}" + ("/mc" if info.get("mc") else "") + ("/sweep" if info.get("sweep") else "")


def caller_driven(q, s, recs, params, plan, first_frame, ticks, want):
    """The loop a caller drives himself: G.caller_loop around ismpc_solve_batch single ticks, every one of which ran the kernel family
    `want`.  Returns (traj [ticks, B], final state, family)."""
    fam = []

    def solve(st):
        out = s.solve_batch(st.view(q.TICK_IN))
        fam.append(family_of(s))
        return out
    traj, fin = G.caller_loop(solve, recs, plan, params.control_dt, params.mpc_dt, first_frame, ticks)
    assert set(fam) == {want}, (set(fam), want)
    return np.stack(traj), fin, fam[0]


def per_tick_family(lanes, sweep=False):
    """What one tick of 13 instances runs on a lane-group handle: a plain handle's batch is resident (ismpc_tick_quad_inline), a sweep
    handle has no resident instantiation and takes the one-launch form (ismpc_tick_quad_one)."""
    return f"quad_one/{lanes}/sweep" if sweep else f"quad_inline/{lanes}"


def rel_com(o, r):
    return np.abs(o["com_pos"] - r["com_pos"]).max(-1) / np.maximum(np.abs(r["com_pos"]).max(-1), 1e-3)


def check_against_oracle(q, name, label, recs, traj, fin):
    """Assertions 2 to 5 of a run WITHOUT pushes: gate bits on every tick of every instance, status / CoM / velocity where the oracle has
    no QP error bit (and up to compare_upto), byte pass-through on gated ticks, the counters of the final state."""
    sc, d = G.SCENARIOS[name], G.scenario(name)
    k = sc["start"]
    upto = G.compare_upto(name) - k                                 # from the oracle alone, before any device result is read
    ref = d["outs"][k:]
    assert traj.shape == ref.shape == (sc["ticks"] - k, B)
    # 2. gate bits: integer decisions, no tolerance
    assert np.array_equal(traj["status"] & G.GATE_BITS, ref["status"] & G.GATE_BITS), \
        (label, np.argwhere((traj["status"] ^ ref["status"]) & G.GATE_BITS)[:5])
    # 3. status, CoM, velocity
    cmp_ = ((ref["status"] & G.QP_ERRORS) == 0) & (np.arange(len(ref))[:, None] < upto[None, :])
    assert np.array_equal(traj["status"][cmp_], ref["status"][cmp_]), (label, np.argwhere(cmp_ & (traj["status"] != ref["status"]))[:5])
    e_com = rel_com(traj, ref)[cmp_].max()
    e_vel = np.abs(traj["com_vel"] - ref["com_vel"]).max(-1)[cmp_].max()
    e_u0 = (np.abs(traj["u0"] - ref["u0"]) / np.maximum(np.abs(ref["u0"]), 1.0)).max(-1)[cmp_].max()
    st = traj["status"]
    counts = {int(v): int((st == v).sum()) for v in np.unique(st)}
    print(f"gates[{name}, {label}]: ticks by status {counts}; max rel CoM {e_com:.2e}, max abs vel {e_vel:.2e}, max u0 {e_u0:.2e} "
          f"over {int(cmp_.sum())} of {cmp_.size} records")
    assert e_com <= TOL and e_vel <= VEL_TOL, (label, e_com, e_vel)
    # 4. pass-through: the record of a gated tick holds the bytes of the state before it (the previous record: every tick is fed back)
    pre_pos = np.concatenate([recs["com_pos"][None], traj["com_pos"][:-1]])
    pre_vel = np.concatenate([recs["com_vel"][None], traj["com_vel"][:-1]])
    gated = (st & G.GATE_BITS) != 0
    assert gated.sum() >= (sc["ticks"] - sc["first_bad"]) * B // 2
    assert traj["com_pos"][gated].tobytes() == pre_pos[gated].tobytes() and traj["com_vel"][gated].tobytes() == pre_vel[gated].tobytes(), label
    assert traj["u0"][gated].tobytes() == np.zeros((int(gated.sum()), 3)).tobytes() and (traj["iters"][gated] == 0).all(), label
    # 5. the final state record
    for f in COUNTERS:
        assert np.array_equal(fin[f], d["fin"][f]), (label, f, fin[f], d["fin"][f])
    assert fin["com_pos"].tobytes() == traj["com_pos"][-1].tobytes() and fin["com_vel"].tobytes() == traj["com_vel"][-1].tobytes()
    if name == "end100":
        assert (fin["control_iter"][0], fin["mpc_iter"][0], fin["footstep_counter"][0]) == (37, 37, 6)


def check_summary(q, name, summ, traj):
    """Assertion 7."""
    sc = G.SCENARIOS[name]
    assert_summary_equal(summ, reduce_summary(q, traj))
    assert (summ["first_error_tick"] == sc["first_bad"] - sc["start"]).all(), summ["first_error_tick"]
    n_bad = ((G.scenario(name)["outs"]["status"][sc["start"]:] & q.ST_BAD_INDEX) != 0).sum(axis=0)
    assert np.array_equal(summ["error_ticks"], n_bad) and (n_bad > 0).all()
    want = q.ST_BAD_INDEX | (q.ST_TICK_SKIPPED if sc["mpc_dt"] != 0.01 else 0)
    assert ((summ["status_or"] & G.GATE_BITS) == want).all(), summ["status_or"]


def gate_pushes(q, name):
    """Two entries per instance: one in front of a tick that runs, one in front of a tick that is skipped (gate*) or carries BAD_INDEX
    (end*; odd instances of gate*), chosen from the oracle's statuses.  Small (0.01 m/s); ticks count from the call's tick 0."""
    sc = G.SCENARIOS[name]
    st = G.scenario(name)["outs"]["status"][sc["start"]:]
    uniform = lambda bit: np.flatnonzero(((st & G.GATE_BITS) == bit).all(axis=1))      # noqa: E731  (ticks where every instance has that gate verdict)
    runs, bad = uniform(0), uniform(q.ST_BAD_INDEX)
    skipped = uniform(q.ST_TICK_SKIPPED) if sc["mpc_dt"] != 0.01 else bad
    rng = np.random.default_rng(7)
    p = np.zeros((B, 2), dtype=q.PUSH)
    p["tick"][:, 0] = runs[runs > 20][:B]                          # a different running tick per instance
    p["tick"][:, 1] = np.where(np.arange(B) % 2 == 0, skipped[skipped > 60][3], bad[2])
    p["dv"] = rng.uniform(-0.01, 0.01, (B, 2, 3)) * np.array([1.0, 1.0, 0.2])
    assert (p["tick"][:, 0] < p["tick"][:, 1]).all() and p["tick"].max() < len(st)
    return p


def run_all_mc_forms(q, name, label, s, s_host, recs, first, ticks, traj, fin, tick_family):
    """Assertions 6 and 7 of the disturbed entry point on one handle pair (loop in the kernel | one launch per tick; s_host None: the
    handle has no in-kernel loop, `s` IS the per-tick form).  tick_family: what one launch per tick runs."""
    kernel = s_host is not None
    t1, s1, f1 = run_mc(q, s, recs, ticks, expect_kernel=kernel, first_frame=first)
    if not kernel:
        assert family_of(s) == tick_family, (family_of(s), tick_family)
    print(f"gates[{name}, {label}]: rollout_mc_torch ran {family_of(s)}")
    assert t1.tobytes() == traj.tobytes() and f1.tobytes() == fin.tobytes()           # MC without pushes == the plain rollout
    check_summary(q, name, s1, traj)
    t7, s7, f7 = run_mc(q, s, recs, ticks, stride=7, expect_kernel=kernel, first_frame=first)
    assert ticks % 7 != 0 and t7.tobytes() == traj[6::7][:ticks // 7].tobytes() and f7.tobytes() == fin.tobytes()
    assert_summary_equal(s7, s1)
    pushes = gate_pushes(q, name)
    ref_traj, ref_fin = segmented(q, s, recs, pushes, ticks, first_frame=first)
    tp, sp, fp = run_mc(q, s, recs, ticks, pushes=pushes, expect_kernel=kernel, first_frame=first)
    assert tp.tobytes() != traj.tobytes()
    for i in range(B):
        assert tp[:, i].tobytes() == ref_traj[:, i].tobytes(), (label, i, pushes["tick"][i])
    assert fp.tobytes() == ref_fin.tobytes()
    assert_summary_equal(sp, reduce_summary(q, tp))
    # the entry in front of a tick that does not run: the record passes the PUSHED state through, and the counters still advance
    for i in range(B):
        t = pushes["tick"][i, 1]
        assert tp["status"][t, i] & G.GATE_BITS and tp["com_pos"][t, i].tobytes() == tp["com_pos"][t - 1, i].tobytes()
        assert tp["com_vel"][t, i].tobytes() == (tp["com_vel"][t - 1, i] + pushes["dv"][i, 1]).tobytes()
    for f in COUNTERS:
        assert np.array_equal(fp[f], fin[f]), f
    if kernel:
        for args in (dict(), dict(stride=7), dict(pushes=pushes)):
            th, sh, fh = run_mc(q, s_host, recs, ticks, expect_kernel=False, first_frame=first, **args)
            want = {"": (t1, s1, f1), "stride": (t7, s7, f7), "pushes": (tp, sp, fp)}[next(iter(args), "")]
            assert th.tobytes() == want[0].tobytes() and fh.tobytes() == want[2].tobytes(), (label, args.keys())
            assert_summary_equal(sh, want[1])
            assert family_of(s_host) == tick_family, (family_of(s_host), tick_family)
        print(f"gates[{name}, {label}]: one launch per tick ran {family_of(s_host)} (ismpc_mc_push / ismpc_mc_fold around it)")


# ---- 1. the lane-group kernels: loop in the kernel == one launch per tick == caller-driven loop, and all of them against the oracle -----------
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", ["end100", "end50", "gate100", "gate50"])
def test_plan_end_and_gated_ticks(q, O, name, lanes):
    sc, d = G.SCENARIOS[name], G.scenario(name)
    G.compare_upto(name)
    first, ticks = sc["start"], sc["ticks"] - sc["start"]
    recs = d["start_state"].view(q.TICK_IN)
    p, plan = device_params(q, name), G.plan(name)
    with Handles(q) as H:
        s, s_host = H.plain(layout(lanes), p, plan), H.plain(layout(lanes, host=True), p, plan)
        traj, fin = run_plain(q, s, recs, ticks, first_frame=first)
        label = f"{lanes} lanes, {family_of(s)}"
        check_against_oracle(q, name, label, recs, traj, fin)
        th, fh = run_plain(q, s_host, recs, ticks, expect_kernel=False, first_frame=first)
        print(f"gates[{name}, {lanes} lanes]: one launch per tick ran {family_of(s_host)}")
        assert family_of(s) == f"rollout_quad/{lanes}" and family_of(s_host) == per_tick_family(lanes)
        assert th.tobytes() == traj.tobytes() and fh.tobytes() == fin.tobytes()
        tc, fc, fam = caller_driven(q, s, recs, p, plan, first, ticks, per_tick_family(lanes))
        print(f"gates[{name}, {lanes} lanes]: caller-driven loop ran {fam}")
        assert tc.tobytes() == traj.tobytes() and fc.tobytes() == fin.tobytes()
        run_all_mc_forms(q, name, label, s, s_host, recs, first, ticks, traj, fin, per_tick_family(lanes))
        assert s.fallback_counters() == (0, 0, 0, 0)


# ---- 2. the forms without an in-kernel loop: one instance per wavefront (N = 150) and the dense path -----------------------------------------
@pytest.mark.parametrize("name,env,family", [("end150", {}, "affine"), ("end100", {"ISMPC_PATH": "dense"}, "dense"),
                                             ("gate100", {"ISMPC_PATH": "dense"}, "dense")])
def test_per_tick_only_forms(q, O, name, env, family):
    sc, d = G.SCENARIOS[name], G.scenario(name)
    G.compare_upto(name)
    first, ticks = sc["start"], sc["ticks"] - sc["start"]
    recs = d["start_state"].view(q.TICK_IN)
    p, plan = device_params(q, name), G.plan(name)
    with Handles(q) as H:
        s = H.plain(env, p, plan)
        traj, fin = run_plain(q, s, recs, ticks, expect_kernel=False, first_frame=first)
        label = family_of(s)
        assert label == f"{family}/64", s.launch_info()
        check_against_oracle(q, name, label, recs, traj, fin)
        tc, fc, fam = caller_driven(q, s, recs, p, plan, first, ticks, label)
        print(f"gates[{name}, {label}]: caller-driven loop ran {fam}")
        assert tc.tobytes() == traj.tobytes() and fc.tobytes() == fin.tobytes()
        run_all_mc_forms(q, name, label, s, None, recs, first, ticks, traj, fin, label)


# ---- 3. a sweep handle of two equal parameter sets (SW = 1): its tables are built on the device, so it meets the others through the oracle ----
@pytest.mark.parametrize("name", ["end100", "gate100"])
def test_sweep_handle(q, O, name):
    sc, d = G.SCENARIOS[name], G.scenario(name)
    G.compare_upto(name)
    first, ticks = sc["start"], sc["ticks"] - sc["start"]
    recs = d["start_state"].view(q.TICK_IN).copy()
    recs["reserved"] = np.arange(B) % 2
    p, plan = device_params(q, name), G.plan(name)
    with Handles(q) as H:
        s = H.sweep({"ISMPC_PATH": "affine"}, [p, device_params(q, name)], plan)
        s_host = H.sweep({"ISMPC_PATH": "affine", "ISMPC_ROLLOUT": "host"}, [p, device_params(q, name)], plan)
        traj, fin = run_plain(q, s, recs, ticks, first_frame=first)
        info = s.launch_info()
        assert info["sweep"] and info["lanes"] == 16, info
        label = family_of(s)
        assert label == "rollout_quad/16/sweep", label
        check_against_oracle(q, name, label, recs, traj, fin)
        assert np.array_equal(fin["reserved"], recs["reserved"])
        th, fh = run_plain(q, s_host, recs, ticks, expect_kernel=False, first_frame=first)
        assert th.tobytes() == traj.tobytes() and fh.tobytes() == fin.tobytes()
        assert family_of(s_host) == per_tick_family(16, sweep=True), family_of(s_host)
        tc, fc, fam = caller_driven(q, s, recs, p, plan, first, ticks, per_tick_family(16, sweep=True))
        print(f"gates[{name}, {label}]: caller-driven loop ran {fam}")
        assert tc.tobytes() == traj.tobytes() and fc.tobytes() == fin.tobytes()
        run_all_mc_forms(q, name, label, s, s_host, recs, first, ticks, traj, fin, per_tick_family(16, sweep=True))


# ---- 4. the NaN guard inside a loop ------------------------------------------------------------------------------------------------------------
def check_guard_tick(q, p, label, rec, z0, zd0):
    """Assertion 8 on one record: the tick whose input carries the NaN.  z = fma(dt, zd0, z0) is NaN on it whichever of the two is
    poisoned, so com_pos[2] is h_des.  zd = fma(dt/m, uz0, zd0) - dt g is NaN as well, also on a poisoned HEIGHT: the force of the
    vertical QP is affine in z0 (the tables of the vertical stage multiply it), so u0[0] is NaN whenever z0 is -- asserted here -- and a
    poisoned height with a finite zd left unreplaced cannot occur."""
    assert rec["status"] == (q.ST_Z_NAN | q.ST_FLIGHT), (label, rec["status"])
    assert np.isnan(z0) or np.isnan(zd0), "scenario: the tick's input is not poisoned"
    assert rec["com_pos"][2].tobytes() == np.float64(p.h_des).tobytes(), (label, rec["com_pos"])
    assert np.isnan(zd0) or np.isnan(rec["u0"][0]), (label, "a NaN height left u0[0] finite", rec["u0"])
    assert rec["com_vel"][2].tobytes() == np.float64(0.0).tobytes(), (label, rec["com_vel"])
    return "z0 NaN" if np.isnan(z0) else "zd0 NaN"


def check_after_guard(q, label, traj, ref, who):
    """Assertion 9: the ticks behind the guard tick, poisoned instances."""
    worst = 0.0
    for i in who:
        o, r = traj[:, i], ref[:, i]
        assert ((o["status"] & q.ST_Z_NAN) == 0).all(), (label, i, o["status"])
        keep = ~(q.ST_X_INFEASIBLE | q.ST_Y_INFEASIBLE)
        assert np.array_equal(o["status"] & keep, r["status"] & keep), (label, i)
        ez = np.abs(o["com_pos"][:, 2] - r["com_pos"][:, 2]) / np.maximum(np.abs(r["com_pos"][:, 2]), 1e-3)
        ezd = np.abs(o["com_vel"][:, 2] - r["com_vel"][:, 2])
        eu = np.abs(o["u0"][:, 0] - r["u0"][:, 0]) / np.maximum(np.abs(r["u0"][:, 0]), 1.0)
        worst = max(worst, ez.max(), ezd.max(), eu.max())
        assert ez.max() <= TOL and ezd.max() <= VEL_TOL and eu.max() <= TOL, (label, i, ez.max(), ezd.max(), eu.max())
        for side in (o, r):
            assert np.isnan(side["com_pos"][:, :2]).all() and np.isnan(side["com_vel"][:, :2]).all(), (label, i)
    return worst


@pytest.mark.parametrize("form", ["lpi8", "lpi16", "lpi32", "dense"])
def test_nan_guard_in_a_loop(q, O, form):
    n = G.nan_case()
    p, plan = device_params(q, "end100"), G.plan("end100")
    who, healthy = G.NAN_Z + G.NAN_ZD, [i for i in range(B) if i not in G.NAN_Z + G.NAN_ZD]
    dense = form == "dense"
    env = {"ISMPC_PATH": "dense"} if dense else layout(int(form[3:]))
    poisoned, clean = n["poisoned"].view(q.TICK_IN), n["clean"].view(q.TICK_IN)
    with Handles(q) as H:
        s = H.plain(env, p, plan)
        s_host = None if dense else H.plain(dict(env, ISMPC_ROLLOUT="host"), p, plan)
        # plain rollouts from the poisoned state
        traj, fin = run_plain(q, s, poisoned, G.NAN_TICKS, expect_kernel=not dense, first_frame=G.NAN_CLEAN)
        label = f"{form}, {family_of(s)}"
        kinds = {i: check_guard_tick(q, p, label, traj[0, i], poisoned["com_pos"][i, 2], poisoned["com_vel"][i, 2]) for i in who}
        worst = check_after_guard(q, label, traj[1:], n["outs"][1:], who)
        print(f"gates[nan100, {label}]: guard tick {kinds}; later ticks max err (z rel, zd abs, u0[0] rel) {worst:.2e}; "
              f"z after {G.NAN_TICKS} ticks {traj['com_pos'][-1, who[0], 2]:.4f}")
        t0, f0 = run_plain(q, s, clean, G.NAN_TICKS, expect_kernel=not dense, first_frame=G.NAN_CLEAN)
        assert traj[:, healthy].tobytes() == t0[:, healthy].tobytes() and fin[healthy].tobytes() == f0[healthy].tobytes()   # 10. neighbours
        assert rel_com(t0, n["healthy_outs"]).max() <= TOL
        tc, fc, fam = caller_driven(q, s, poisoned, p, plan, G.NAN_CLEAN, G.NAN_TICKS, "dense/64" if dense else per_tick_family(int(form[3:])))
        assert tc.tobytes() == traj.tobytes() and fc.tobytes() == fin.tobytes()                    # NaN payloads included
        if s_host:
            th, fh = run_plain(q, s_host, poisoned, G.NAN_TICKS, expect_kernel=False, first_frame=G.NAN_CLEAN)
            assert family_of(s_host) == per_tick_family(int(form[3:])), family_of(s_host)
            assert th.tobytes() == traj.tobytes() and fh.tobytes() == fin.tobytes()
        for f in COUNTERS:
            assert np.array_equal(fin[f], n["fin"][f]), f
        # the disturbed loop reaches the state from inside: dv[2] = NaN in front of tick 30 of 70
        ticks, recs = G.NAN_CLEAN + G.NAN_TICKS, n["recs"].view(q.TICK_IN)
        pushes = G.nan_pushes(q.PUSH)
        tm, sm, fm = run_mc(q, s, recs, ticks, pushes=pushes, expect_kernel=not dense)
        for i in who:
            zd0 = tm["com_vel"][G.NAN_CLEAN - 1, i, 2] + pushes["dv"][i, 0, 2]
            check_guard_tick(q, p, label + " mc", tm[G.NAN_CLEAN, i], tm["com_pos"][G.NAN_CLEAN - 1, i, 2], zd0)
        worst = check_after_guard(q, label + " mc", tm[G.NAN_CLEAN + 1:], n["mc_outs"][G.NAN_CLEAN + 1:], who)
        print(f"gates[nan100, {label}]: rollout_mc_torch ran {family_of(s)}; later ticks max err {worst:.2e}")
        t_no, s_no, f_no = run_mc(q, s, recs, ticks, expect_kernel=not dense)
        assert tm[:, healthy].tobytes() == t_no[:, healthy].tobytes() and fm[healthy].tobytes() == f_no[healthy].tobytes()
        assert sm[healthy].tobytes() == s_no[healthy].tobytes()
        assert_summary_equal(sm, reduce_summary(q, tm))                 # np.fmin / np.fmax: NaN records leave the extrema alone
        assert np.isfinite(sm["com_z_min"][list(who)]).all() and np.isfinite(sm["com_z_max"][list(who)]).all()
        assert np.isfinite(sm["max_abs_vel"]).all() and (sm["status_or"][list(who)] & q.ST_Z_NAN).all()
        assert np.array_equal(sm["max_abs_vel"][list(who)], np.abs(tm["com_vel"][:G.NAN_CLEAN, list(who), :2]).max(axis=0))
        if s_host:
            th, sh, fh = run_mc(q, s_host, recs, ticks, pushes=pushes, expect_kernel=False)
            assert th.tobytes() == tm.tobytes() and fh.tobytes() == fm.tobytes()
            assert_summary_equal(sh, sm)
        sg, fg = segmented(q, s, recs, pushes, ticks)
        assert sg.tobytes() == tm.tobytes() and fg.tobytes() == fm.tobytes()


# ---- 5. a vertical solve that fails on every tick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_failed_vertical_solve_is_never_fed_back(q, O, lanes):
    """ISMPC_ST_Z_FAILED: "never fed back in closed loops" (include/ismpc.h).  z_ineq_lo = 1e-3 cannot be met: every instance defers every
    tick, the in-kernel loop parks all of them at tick 0 and the resume launch runs the whole call.  The oracle is a reference for the
    first tick only (it feeds a failed tick back); behind it the device forms are compared with each other and with the header's rule."""
    z = G.zfail_case()
    recs, ticks = z["recs"].view(q.TICK_IN), G.ZFAIL_TICKS
    p = q.default_params(N=100, z_ineq_lo=G.ZFAIL_LO)
    plan = q.reference_plan(params=p)
    with Handles(q) as H:
        s, s_host = H.plain(layout(lanes), p, plan), H.plain(layout(lanes, host=True), p, plan)
        traj, fin = run_plain(q, s, recs, ticks)
        assert ((traj["status"] & q.ST_Z_FAILED) != 0).all(), traj["status"]
        assert np.array_equal(traj["status"][0] & q.ST_Z_FAILED, z["first_tick"]["status"] & q.ST_Z_FAILED)
        assert fin["com_pos"].tobytes() == recs["com_pos"].tobytes() and fin["com_vel"].tobytes() == recs["com_vel"].tobytes()
        print(f"gates[zfail, {lanes} lanes, {family_of(s)}]: statuses {sorted(set(traj['status'].ravel().tolist()))}, final counters "
              f"{[(f, sorted(set(fin[f].tolist()))) for f in COUNTERS]}")
        tm, sm, fm = run_mc(q, s, recs, ticks)
        assert tm.tobytes() == traj.tobytes() and fm.tobytes() == fin.tobytes()
        assert (sm["error_ticks"] == ticks).all() and (sm["first_error_tick"] == 0).all()
        assert_summary_equal(sm, reduce_summary(q, tm))
        th, fh = run_plain(q, s_host, recs, ticks, expect_kernel=False)
        assert family_of(s_host) == per_tick_family(lanes), family_of(s_host)
        assert th.tobytes() == traj.tobytes() and fh.tobytes() == fin.tobytes()
        thm, shm, fhm = run_mc(q, s_host, recs, ticks, expect_kernel=False)
        assert thm.tobytes() == traj.tobytes() and fhm.tobytes() == fin.tobytes()
        assert_summary_equal(shm, sm)
        # tick by tick: a call of one tick leaves com_pos / com_vel as they were
        t1, f1 = run_plain(q, s, recs, 1)
        assert t1.tobytes() == traj[:1].tobytes() and f1["com_pos"].tobytes() == recs["com_pos"].tobytes() and f1["com_vel"].tobytes() == recs["com_vel"].tobytes()
        assert s.fallback_counters() == (0, 0, 0, 0)


def test_failed_vertical_solve_on_the_dense_path(q, O):
    """The dense path (ISMPC_PATH=dense) has no active-set fallback behind its vertical solve: a violated bound on S u is flagged
    ISMPC_ST_Z_INEQ_ACTIVE and the unconstrained solution is what the tick returns.  The header's rule is asserted as a rule, tick by tick
    through memory: a record with ISMPC_ST_Z_FAILED leaves com_pos / com_vel of the state as they were, every other record IS the state
    after the tick."""
    z = G.zfail_case()
    recs, ticks = z["recs"].view(q.TICK_IN), G.ZFAIL_TICKS
    p = q.default_params(N=100, z_ineq_lo=G.ZFAIL_LO)
    with Handles(q) as H:
        s = H.plain({"ISMPC_PATH": "dense"}, p, q.reference_plan(params=p))
        traj, fin = run_plain(q, s, recs, ticks, expect_kernel=False)
        assert family_of(s) == "dense/64", s.launch_info()
        tm, sm, fm = run_mc(q, s, recs, ticks, expect_kernel=False)
        assert tm.tobytes() == traj.tobytes() and fm.tobytes() == fin.tobytes()
        assert_summary_equal(sm, reduce_summary(q, tm))
        state, failed = recs, 0
        for t in range(ticks):
            t1, after = run_plain(q, s, state, 1, expect_kernel=False, first_frame=t)
            assert t1[0].tobytes() == traj[t].tobytes()
            bad = (t1[0]["status"] & q.ST_Z_FAILED) != 0
            want_pos = np.where(bad[:, None], state["com_pos"], t1[0]["com_pos"])
            want_vel = np.where(bad[:, None], state["com_vel"], t1[0]["com_vel"])
            assert after["com_pos"].tobytes() == want_pos.tobytes() and after["com_vel"].tobytes() == want_vel.tobytes(), t
            failed += int(bad.sum())
            state = after
        assert state.tobytes() == fin.tobytes()
        assert ((traj["status"] & q.ST_Z_INEQ_ACTIVE) != 0).all()
        print(f"gates[zfail, {family_of(s)}]: statuses {sorted(set(traj['status'].ravel().tolist()))}, records with Z_FAILED {failed} of {traj.size}")
