"""GPU tests of the disturbed closed loop (ismpc_rollout_mc_device): per-instance velocity pushes in front of a tick, a trajectory row
every `stride` ticks and one summary per instance, inside one launch (ismpc_rollout_quad, MC = true).

The references are independent of the code under test: the PLAIN rollout (ismpc_rollout_device, the MC = false kernels) run in segments
with torch adding dv to the state between them; the same call on a handle that runs one launch per tick (ISMPC_ROLLOUT=host: two small
elementwise kernels around the tick); a numpy reduction of the trajectory for the summary; and the CPU oracle driven in segments.
Everything but the oracle comparison is byte for byte.  The cursor rule of include/ismpc.h is restated here in Python (applied_entries).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-6                      # the project's relative CoM tolerance (tests/test_gpu_parity.py)
B = 37                          # a partial last wavefront and more than one workgroup at 8, 16 and 32 lanes per instance
INT32_MAX = 2 ** 31 - 1
LANES = (8, 16, 32)
# name: (N, ticks, parameter overrides).  The tight z_ineq_hi values make the vertical inequality rows active around tick 87: the
# instance is parked by the first launch and resumed by the second
CASES = {"N100": (100, 200, {}), "N50": (50, 150, {}), "N100z": (100, 200, dict(z_ineq_hi=5.0)), "N50z": (50, 150, dict(z_ineq_hi=1.3))}
FREE, PARKED = ("N100", "N50"), ("N100z", "N50z")


@pytest.fixture(scope="module")
def q(built_libs):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import quadruped_gait_generation_ismpc_amd as q
    return q


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


_KNOBS = ("ISMPC_PATH", "ISMPC_LPI", "ISMPC_ROLLOUT", "ISMPC_ONE_LAUNCH", "ISMPC_Z_FALLBACK")
_solvers = {}


def make_under(env, make):
    """make() with exactly these knobs in the environment (a handle reads them when it is created)."""
    saved = {k: os.environ.pop(k, None) for k in _KNOBS}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def solver_for(q, case, lanes, host=False):
    """The shared handle of (case, lanes per instance, in-kernel loop | one launch per tick)."""
    key = (case, lanes, host)
    if key not in _solvers:
        N, _, over = CASES[case]
        p = q.default_params(N=N, **over)
        env = {"ISMPC_PATH": "affine", "ISMPC_LPI": str(lanes)}
        if host:
            env["ISMPC_ROLLOUT"] = "host"
        _solvers[key] = make_under(env, lambda: q.MPCSolver(q.reference_plan(params=p), params=p))
    return _solvers[key]


def initial_records(q, O, n=B):
    """The reference's initial state, perturbed per instance as in test_in_kernel_rollout_is_bitwise_the_per_tick_loop."""
    recs = np.repeat(O.initial_state().view(q.TICK_IN), n)
    rng = np.random.default_rng(9)
    recs["com_pos"][1:, :2] += rng.uniform(-0.004, 0.004, (n - 1, 2))
    recs["com_vel"][1:, :2] += rng.uniform(-0.02, 0.02, (n - 1, 2))
    return recs


def applied_entries(ticks_of_table, ticks):
    """The cursor rule: at tick t the cursor advances over every entry whose tick <= t and applies those whose tick == t.  Returns
    [(t, j)] in the order the entries apply."""
    cur, n, res = 0, len(ticks_of_table), []
    for t in range(ticks):
        while cur < n and ticks_of_table[cur] <= t:
            if ticks_of_table[cur] == t:
                res.append((t, cur))
            cur += 1
    return res


def random_pushes(q, n, n_push, pool, seed, scale=(0.05, 0.05, 0.02)):
    """n_push entries per instance at ticks drawn from `pool` (ascending per instance), dv uniform within +-scale."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, n_push), dtype=q.PUSH)
    p["tick"] = np.sort(rng.choice(pool, (n, n_push)), axis=1)
    p["dv"] = rng.uniform(-1.0, 1.0, (n, n_push, 3)) * np.array(scale)
    return p


def push_tensor(q, pushes):
    return q.to_device(pushes.reshape(-1)).view(pushes.shape[0], pushes.shape[1], 32)


def run_mc(q, s, recs, ticks, pushes=None, stride=1, want_traj=True, want_summary=True, expect_kernel=True, first_frame=0):
    """One call of the entry point under test.  Returns (trajectory records or None, summary records or None, final state records)."""
    import torch
    st = q.to_device(recs)
    traj, summ = s.rollout_mc_torch(st, first_frame, ticks, pushes=None if pushes is None else push_tensor(q, pushes), stride=stride,
                                    want_traj=want_traj, want_summary=want_summary)
    torch.cuda.synchronize()
    info = s.launch_info()
    if expect_kernel:
        assert info["family"] == "rollout_quad" and info.get("mc") is True and info["kernels"] == 2 and info["batch"] == len(recs), info
    else:
        assert info["family"] != "rollout_quad" and "mc" not in info, info
    return (None if traj is None else q.from_device(traj, q.TICK_OUT), None if summ is None else q.from_device(summ, q.ROLLOUT_SUMMARY),
            q.from_device(st, q.TICK_IN))


def run_plain(q, s, recs, ticks, expect_kernel=True, first_frame=0):
    import torch
    st = q.to_device(recs)
    traj = s.rollout_torch(st, first_frame, ticks)
    torch.cuda.synchronize()
    info = s.launch_info()
    assert (info["family"] == "rollout_quad") == expect_kernel and "mc" not in info, info
    return q.from_device(traj, q.TICK_OUT), q.from_device(st, q.TICK_IN)


def segmented(q, s, recs, pushes, ticks, first_frame=0):
    """The reference computation: plain rollouts (ismpc_rollout_device) between the push ticks, torch adding dv to the com_vel bytes of
    the state tensor in between -- one fp64 add per component and entry, in the order the cursor rule applies them.  (Push ticks count
    from the call's tick 0, frames from first_frame.)"""
    import torch
    st = q.to_device(recs)
    v = st.view(torch.float64)                                   # [B, 9]: com_pos, com_vel, simulation_time, counters
    events = {}                                                  # tick -> levels -> [(instance, entry)]: level k = the k-th entry of an instance at that tick
    for i in range(len(recs)):
        seen = {}
        for t, j in applied_entries(pushes["tick"][i], ticks):
            k = seen.get(t, 0); seen[t] = k + 1
            events.setdefault(t, {}).setdefault(k, []).append((i, j))
    parts, a = [], 0
    for b in sorted(events):
        if b > a:
            parts.append(s.rollout_torch(st, first_frame + a, b - a))
        for k in sorted(events[b]):
            idx = torch.tensor([i for i, _ in events[b][k]], device=st.device)
            dv = torch.tensor(np.stack([pushes["dv"][i, j] for i, j in events[b][k]]), device=st.device)
            v[idx, 3:6] = v[idx, 3:6] + dv
        a = b
    parts.append(s.rollout_torch(st, first_frame + a, ticks - a))
    torch.cuda.synchronize()
    return q.from_device(torch.cat(parts), q.TICK_OUT), q.from_device(st, q.TICK_IN)


_nominal = {}


def nominal(q, O, case, lanes):
    """The undisturbed plain rollout of the shared initial records (computed once per case and layout, never changed)."""
    key = (case, lanes)
    if key not in _nominal:
        _, ticks, _ = CASES[case]
        recs = initial_records(q, O)
        traj, fin = run_plain(q, solver_for(q, case, lanes), recs, ticks)
        for a in (recs, traj, fin):
            a.setflags(write=False)
        _nominal[key] = (recs, traj, fin)
    return _nominal[key]


def fixed_case_pushes(q, case, traj):
    """Test 2's table: three random pushes per instance, and on instances 0..7 the fixed cases."""
    _, ticks, _ = CASES[case]
    pool = np.array([5, 17, 33, 48, 64, 85, 97, 110, 126, 140])
    p = random_pushes(q, B, 3, pool, seed=101)
    flight = np.flatnonzero(traj["status"][:, 4] & q.ST_FLIGHT)
    assert len(flight), "the undisturbed run of instance 4 has no flight tick"
    fixed = {0: (0, 48, 97),                       # tick 0
             1: (33, 64, ticks - 1),               # the last tick
             2: (40, 41, 42),                      # three consecutive ticks
             3: (50, 50, 110),                     # two entries on one tick
             4: (17, int(flight[len(flight) // 2]), 140),      # a tick in the flight phase of the undisturbed run
             5: (85, 30, 126),                     # unsorted: the entry at 30 sits behind 85 and is skipped
             6: (-5, 20, 64),                      # a negative tick never applies
             7: (10, 97, ticks)}                   # nor does a tick equal to `ticks`
    for i, tk in fixed.items():
        p["tick"][i] = tk
    assert [t for t, _ in applied_entries(p["tick"][5], ticks)] == [85, 126] and len(applied_entries(p["tick"][3], ticks)) == 3
    assert len(applied_entries(p["tick"][6], ticks)) == 2 and len(applied_entries(p["tick"][7], ticks)) == 2
    return p


def park_pushes(q, case, traj):
    """Test 3's table: each instance's park tick from the undisturbed run's first ISMPC_ST_Z_INEQ_ACTIVE; instances pushed at park - 1,
    park, park + 1, park + 30 in turn, every other one also 0.03 m/s at tick 50 (which leaves the park tick where it is)."""
    act = (traj["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    assert act.any(axis=0).all(), "an instance never parks in the undisturbed run"
    park = act.argmax(axis=0)
    assert (park >= 60).all() and (park + 30 < traj.shape[0]).all(), park
    rng = np.random.default_rng(202)
    p = np.zeros((B, 2), dtype=q.PUSH)
    p["tick"][:, 0] = np.where(np.arange(B) % 2 == 0, 50, -1)
    p["dv"][:, 0, :2] = 0.03 * np.sign(rng.uniform(-1, 1, (B, 2)))
    p["tick"][:, 1] = park + np.array([-1, 0, 1, 30])[np.arange(B) % 4]
    p["dv"][:, 1] = rng.uniform(-1.0, 1.0, (B, 3)) * np.array([0.05, 0.05, 0.02])
    return p


def summary_pushes(q):
    """Test 5's table: 0.3 m/s (x, -y) on the even instances, at tick 60, 83 or 100."""
    p = np.zeros((B, 1), dtype=q.PUSH)
    p["tick"][:, 0] = INT32_MAX
    even = np.arange(0, B, 2)
    p["tick"][even, 0] = np.array([60, 83, 100])[(even // 2) % 3]
    p["dv"][even, 0] = (0.3, -0.3, 0.0)
    return p


def reduce_summary(q, traj):
    """The summary as a numpy reduction of a stride-1 trajectory [ticks, B]."""
    st = traj["status"]
    s = np.zeros(traj.shape[1], dtype=q.ROLLOUT_SUMMARY)
    s["status_or"] = np.bitwise_or.reduce(st, axis=0)
    err = (st & q.ST_ERROR_MASK) != 0
    s["first_error_tick"] = np.where(err.any(axis=0), err.argmax(axis=0), -1)
    s["error_ticks"] = err.sum(axis=0)
    s["fallback_ticks"] = ((st & q.ST_Z_INEQ_ACTIVE) != 0).sum(axis=0)
    s["com_z_min"] = np.fmin.reduce(traj["com_pos"][:, :, 2], axis=0)
    s["com_z_max"] = np.fmax.reduce(traj["com_pos"][:, :, 2], axis=0)
    s["max_abs_vel"] = np.fmax.reduce(np.abs(traj["com_vel"][:, :, :2]), axis=0, initial=0.0)
    return s


def assert_summary_equal(a, b):
    for name in a.dtype.names:                                   # field by field; the doubles by their bytes
        assert a[name].tobytes() == b[name].tobytes(), (name, a[name], b[name])


# ---- 1. no disturbance is the plain rollout
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", FREE + PARKED)
def test_no_disturbance_is_the_plain_rollout(q, O, case, lanes):
    _, ticks, _ = CASES[case]
    recs, traj, fin = nominal(q, O, case, lanes)
    s = solver_for(q, case, lanes)
    t1, _, f1 = run_mc(q, s, recs, ticks, want_summary=False)
    assert t1.tobytes() == traj.tobytes() and f1.tobytes() == fin.tobytes()
    pad = np.zeros((B, 3), dtype=q.PUSH)
    pad["tick"] = INT32_MAX
    pad["dv"] = 1.0                                              # would be seen if it were ever applied
    t2, _, f2 = run_mc(q, s, recs, ticks, pushes=pad)
    assert t2.tobytes() == traj.tobytes() and f2.tobytes() == fin.tobytes()
    assert s.fallback_counters() == (0, 0, 0, 0)


# ---- 2. pushes, bit for bit against segmented plain rollouts (and 4.: against one launch per tick)
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", FREE)
def test_pushes_are_bitwise_the_segmented_plain_rollout(q, O, case, lanes):
    _, ticks, _ = CASES[case]
    recs, traj0, _ = nominal(q, O, case, lanes)
    pushes = fixed_case_pushes(q, case, traj0)
    s = solver_for(q, case, lanes)
    ref_traj, ref_fin = segmented(q, s, recs, pushes, ticks)
    traj, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    assert traj.shape == ref_traj.shape == (ticks, B)
    assert (traj.tobytes() != traj0.tobytes())                   # the pushes do change the run
    for i in range(B):
        assert traj[:, i].tobytes() == ref_traj[:, i].tobytes(), (i, pushes["tick"][i])
    assert fin.tobytes() == ref_fin.tobytes()
    # 4. the same call as one launch per tick: trajectory, final state and summary
    h_traj, h_summ, h_fin = run_mc(q, solver_for(q, case, lanes, host=True), recs, ticks, pushes=pushes, expect_kernel=False)
    assert h_traj.tobytes() == traj.tobytes() and h_fin.tobytes() == fin.tobytes()
    assert_summary_equal(summ, h_summ)
    assert_summary_equal(summ, reduce_summary(q, traj))


# ---- 3. parked instances: pushes around the park tick (and 4. again)
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", PARKED)
def test_pushes_around_the_park_tick(q, O, case, lanes):
    _, ticks, _ = CASES[case]
    recs, traj0, _ = nominal(q, O, case, lanes)
    pushes = park_pushes(q, case, traj0)
    s = solver_for(q, case, lanes)
    ref_traj, ref_fin = segmented(q, s, recs, pushes, ticks)
    traj, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    for i in range(B):
        assert traj[:, i].tobytes() == ref_traj[:, i].tobytes(), (i, pushes["tick"][i])
    assert fin.tobytes() == ref_fin.tobytes()
    assert ((traj["status"] & q.ST_Z_INEQ_ACTIVE) != 0).any(axis=0).all()       # every instance went through the resume launch
    assert s.fallback_counters() == (0, 0, 0, 0)
    h_traj, h_summ, h_fin = run_mc(q, solver_for(q, case, lanes, host=True), recs, ticks, pushes=pushes, expect_kernel=False)
    assert h_traj.tobytes() == traj.tobytes() and h_fin.tobytes() == fin.tobytes()
    assert_summary_equal(summ, h_summ)
    assert (summ["fallback_ticks"] > 0).all()


# ---- 5. the summary against a numpy reduction of the trajectory
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", ["N100", "N100z"])
def test_summary_is_the_reduction_of_the_trajectory(q, O, case, lanes):
    _, ticks, _ = CASES[case]
    recs = initial_records(q, O)
    pushes = summary_pushes(q)
    s = solver_for(q, case, lanes)
    traj, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    assert_summary_equal(summ, reduce_summary(q, traj))
    pushed = pushes["tick"][:, 0] < ticks
    assert pushed.sum() == (B + 1) // 2
    # a 0.3 m/s shove makes the horizontal QPs infeasible (on the CPU oracle from tick 60, 90 and 100 on): the data are not all clean
    assert (summ["error_ticks"][pushed] > 0).all(), summ["error_ticks"]
    assert (summ["first_error_tick"][pushed] >= pushes["tick"][pushed, 0]).all()
    assert (summ["first_error_tick"][~pushed] == -1).all() and (summ["error_ticks"][~pushed] == 0).all()
    if case in PARKED:
        assert (summ["fallback_ticks"] > 0).all()                # partial summaries crossed the park
    else:
        assert (summ["fallback_ticks"] == 0).all()
    # without a trajectory buffer: same summary, same final state; without a summary: same trajectory
    _, s2, f2 = run_mc(q, s, recs, ticks, pushes=pushes, want_traj=False)
    assert_summary_equal(summ, s2)
    assert f2.tobytes() == fin.tobytes()
    t3, s3, f3 = run_mc(q, s, recs, ticks, pushes=pushes, want_summary=False)
    assert s3 is None and t3.tobytes() == traj.tobytes() and f3.tobytes() == fin.tobytes()
    # and as one launch per tick
    h_traj, h_summ, h_fin = run_mc(q, solver_for(q, case, lanes, host=True), recs, ticks, pushes=pushes, expect_kernel=False)
    assert h_traj.tobytes() == traj.tobytes() and h_fin.tobytes() == fin.tobytes()
    assert_summary_equal(summ, h_summ)
    _, h2, hf2 = run_mc(q, solver_for(q, case, lanes, host=True), recs, ticks, pushes=pushes, want_traj=False, expect_kernel=False)
    assert_summary_equal(summ, h2)
    assert hf2.tobytes() == fin.tobytes()
    assert s.fallback_counters() == (0, 0, 0, 0)


# ---- 6. stride
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", ["N100", "N100z", "N50z"])
def test_trajectory_stride(q, O, case, lanes):
    _, ticks, _ = CASES[case]
    recs, traj0, _ = nominal(q, O, case, lanes)
    pushes = park_pushes(q, case, traj0) if case in PARKED else random_pushes(q, B, 3, np.array([5, 48, 85, 126]), seed=303)
    s = solver_for(q, case, lanes)
    full, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    t7, s7, f7 = run_mc(q, s, recs, ticks, pushes=pushes, stride=7)
    assert t7.shape == (ticks // 7, B) and ticks % 7 != 0        # 200 ticks: 28 rows and 4 ticks left over
    assert t7.tobytes() == full[6::7][:ticks // 7].tobytes()
    assert_summary_equal(summ, s7)
    assert f7.tobytes() == fin.tobytes()
    h7, hs7, hf7 = run_mc(q, solver_for(q, case, lanes, host=True), recs, ticks, pushes=pushes, stride=7, expect_kernel=False)
    assert h7.tobytes() == t7.tobytes() and hf7.tobytes() == fin.tobytes()
    assert_summary_equal(summ, hs7)
    # a stride beyond the call: no row at all, the summary and the final state are still those
    t_none, s_big, f_big = run_mc(q, s, recs, ticks, pushes=pushes, stride=ticks + 1)
    assert t_none.shape == (0, B) and f_big.tobytes() == fin.tobytes()
    assert_summary_equal(summ, s_big)


# ---- 7. against the CPU oracle, driven in segments
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", FREE)
def test_against_the_oracle_in_segments(q, O, case, lanes):
    N, ticks, over = CASES[case]
    n = 16
    recs = initial_records(q, O, n)
    ref = _oracle_reference(q, O, case)
    traj, summ, fin = run_mc(q, solver_for(q, case, lanes), recs, ticks, pushes=ref["pushes"])
    worst = 0.0
    for i in range(n):
        o, r = traj[:, i], ref["outs"][i]
        assert np.array_equal(o["status"], r["status"]), (i, np.flatnonzero(o["status"] != r["status"])[:5])
        rel = np.abs(o["com_pos"] - r["com_pos"]).max(1) / np.maximum(np.abs(r["com_pos"]).max(1), 1e-3)
        worst = max(worst, rel.max())
        assert rel.max() <= TOL and np.abs(o["com_vel"] - r["com_vel"]).max() <= TOL, (i, rel.max())
        for k in ("mpc_iter", "control_iter", "footstep_counter", "simulation_time"):
            assert fin[k][i] == ref["fin"][i][k][0], (i, k)     # counters bit exact
    print(f"oracle[{case}, {lanes} lanes]: max rel CoM err {worst:.2e}")
    assert (summ["first_error_tick"] == -1).all()


_oracle_ref = {}


def _oracle_reference(q, O, case):
    """Sixteen instances, three pushes each (+-0.05 m/s in x and y, +-0.02 in z; among them ticks 0, the last one and 40, 41, 42):
    Oracle.rollout up to the push tick, dv added to the returned state, continued at the next frame.  Computed once per case."""
    if case not in _oracle_ref:
        N, ticks, over = CASES[case]
        n = 16
        recs = initial_records(q, O, n)
        pushes = random_pushes(q, n, 3, np.array([5, 17, 33, 48, 64, 85, 97, 110, 126, 140]), seed=404)
        pushes["tick"][0] = (0, 64, ticks - 1)
        pushes["tick"][1] = (40, 41, 42)
        orc = O.Oracle(O.default_params(N, **over))
        outs, fins = [], []
        for i in range(n):
            st, a, parts = recs[i:i + 1].copy(), 0, []
            ev = applied_entries(pushes["tick"][i], ticks)
            for b in sorted(set(t for t, _ in ev)):
                if b > a:
                    o, _, _, st = orc.rollout(st, a, b - a)
                    parts.append(o)
                st = st.copy()
                for t, j in ev:
                    if t == b:
                        st["com_vel"][0] = st["com_vel"][0] + pushes["dv"][i, j]
                a = b
            o, _, _, st = orc.rollout(st, a, ticks - a)
            parts.append(o)
            o = np.concatenate(parts)
            # a condition on the inputs: at these magnitudes the oracle's own run carries no error bit, on any instance
            assert (o["status"] & q.ST_ERROR_MASK).sum() == 0, (case, i)
            outs.append(o.view(q.TICK_OUT)); fins.append(st)
        _oracle_ref[case] = dict(pushes=pushes, outs=outs, fin=fins)
    return _oracle_ref[case]


# ---- 8. handle kinds
def test_sweep_handle(q, O):
    """Three parameter sets at 16 lanes per instance, the third with a tight bound on S u: its instances park."""
    ticks = 200
    sets = [q.default_params(N=100), q.default_params(N=100, mass=46.0), q.default_params(N=100, z_ineq_hi=5.0)]
    s = make_under({"ISMPC_PATH": "affine"}, lambda: q.MPCSolver.sweep(q.reference_plan(params=sets[0]), sets))
    recs = initial_records(q, O)
    recs["reserved"] = np.arange(B) % 3
    recs["reserved"][B - 1] = 7                                  # names no set: ISMPC_ST_BAD_INDEX, state passed through -- pushes included
    pushes = random_pushes(q, B, 3, np.array([0, 17, 48, 86, 87, 88, 126, 199]), seed=505)
    ref_traj, ref_fin = segmented(q, s, recs, pushes, ticks)
    traj, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    info = s.launch_info()
    assert info["sweep"] and info["lanes"] == 16 and info["mc"], info
    assert traj.tobytes() == ref_traj.tobytes() and fin.tobytes() == ref_fin.tobytes()
    assert_summary_equal(summ, reduce_summary(q, traj))
    parked = (summ["fallback_ticks"] > 0)
    assert parked[2:B - 1:3].all() and not parked[0::3].any() and not parked[1::3].any(), parked
    assert summ["status_or"][B - 1] == q.ST_BAD_INDEX and summ["error_ticks"][B - 1] == ticks and summ["first_error_tick"][B - 1] == 0
    assert s.fallback_counters() == (0, 0, 0, 0)
    s.close()


def test_multi_plan_handle(q, O):
    """Two footstep plans with different step timing in one handle."""
    from quadruped_gait_generation_ismpc_amd import workload
    ticks = 200
    params = q.default_params(N=100)
    plans = workload.make_plans(8, params)
    other = next(p for p in plans[1:] if p[1, 3] != plans[0][1, 3])
    s = make_under({"ISMPC_PATH": "affine", "ISMPC_LPI": "8"}, lambda: q.MPCSolver.plans([plans[0], other], params))
    recs = initial_records(q, O)
    recs["reserved"] = q.pack_reserved(0, np.arange(B) % 2)
    pushes = random_pushes(q, B, 3, np.array([0, 17, 39, 44, 85, 126, 199]), seed=606)
    ref_traj, ref_fin = segmented(q, s, recs, pushes, ticks)
    traj, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    info = s.launch_info()
    assert info.get("plans") and info["mc"] and info["lanes"] == 8, info
    assert traj.tobytes() == ref_traj.tobytes() and fin.tobytes() == ref_fin.tobytes()
    assert_summary_equal(summ, reduce_summary(q, traj))
    assert len(set(fin["footstep_counter"][:2])) == 2 or not np.array_equal(fin["mpc_iter"][0], fin["mpc_iter"][1])      # the plans do step at different ticks
    s.close()


# ---- 9. position independence
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("case", ["N100", "N50z"])
def test_position_independence(q, O, case, lanes):
    _, ticks, _ = CASES[case]
    recs, traj0, _ = nominal(q, O, case, lanes)
    pushes = park_pushes(q, case, traj0) if case in PARKED else fixed_case_pushes(q, case, traj0)
    s = solver_for(q, case, lanes)
    traj, summ, fin = run_mc(q, s, recs, ticks, pushes=pushes)
    perm = np.random.default_rng(0).permutation(B)
    tp, sp, fp = run_mc(q, s, recs[perm], ticks, pushes=pushes[perm])
    assert tp.tobytes() == np.ascontiguousarray(traj[:, perm]).tobytes()
    assert fp.tobytes() == fin[perm].tobytes()
    assert_summary_equal(sp, summ[perm])
    # and a smaller batch: an instance's bytes do not depend on the others (one workgroup, a partial wavefront)
    t5, s5, f5 = run_mc(q, s, recs[:5], ticks, pushes=pushes[:5])
    assert t5.tobytes() == np.ascontiguousarray(traj[:, :5]).tobytes() and f5.tobytes() == fin[:5].tobytes()
    assert_summary_equal(s5, summ[:5])


def test_empty_calls_and_reserve(q, O):
    """ticks = 0 gives the empty summary and leaves the state alone; batch = 0 is a no-op; ismpc_reserve sizes the scratch record."""
    s = solver_for(q, "N100", 16)
    s.reserve(64)
    recs = initial_records(q, O, 5)
    import torch
    st = q.to_device(recs)
    traj, summ = s.rollout_mc_torch(st, 0, 0)
    torch.cuda.synchronize()
    sm = q.from_device(summ, q.ROLLOUT_SUMMARY)
    assert traj.shape[0] == 0 and q.from_device(st, q.TICK_IN).tobytes() == recs.tobytes()
    assert (sm["status_or"] == 0).all() and (sm["first_error_tick"] == -1).all() and (sm["error_ticks"] == 0).all() and (sm["fallback_ticks"] == 0).all()
    assert np.isposinf(sm["com_z_min"]).all() and np.isneginf(sm["com_z_max"]).all() and (sm["max_abs_vel"] == 0).all()
    e = torch.empty((0, 72), dtype=torch.uint8, device="cuda:0")
    s.rollout_mc_torch(e, 0, 10)
    torch.cuda.synchronize()
