"""Multi-plan handles of Formulation B (ismpc_create_plans): the instances of ONE batch walk different footstep plans -- heading, stride,
stance width, step timing -- and, with several parameter sets, different parameters too.  Every comparison is against one CPU oracle
per plan (per (set, plan) pair), built on that plan; with one parameter set the records are byte-identical to a plain handle created on
the instance's plan, in every lane layout and launch form.

The committed pre-rolls follow the reference plan only, so the nominal states come from the oracle's own closed loop on each plan:
260 ticks from the initial state, inputs picked from ticks 20..259 and perturbed with workload.PERTURB at scale 1.  P = 8 plans x 24
instances = 192 is the smallest batch that puts several plans into every wavefront at all three layouts (2, 4 or 8 instances per
wavefront).  Each comparison first asserts that at least 90 % of the sample is compared (no error bit on either side) and that at least
70 % of the compared instances have status 0, i.e. that the horizontal stage did read the plan.
Tolerances as in tests/test_gpu_sweep.py: CoM 1e-6 relative, velocity 1e-6, u0 1e-6 x max(scale, |ref|), status bit-exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-6
P, PER = 8, 24
B = P * PER
LAYOUTS = [None, "8", "16", "32"]                    # ISMPC_LPI: the default dispatch and the three lane layouts


@pytest.fixture(scope="module")
def q(built_libs):
    import torch
    assert torch.cuda.is_available()
    import quadruped_gait_generation_ismpc_amd as q
    return q


def oracle_params(O, N, p=None, **over):
    if p is not None:
        over = dict(mass=p.mass, h_des=p.h_des, q_p=p.q_p, q_u=p.q_u, q_v=p.q_v, foot_width=p.foot_width, **over)
    return O.default_params(N, **over)


def nominal_inputs(q, O, N, plans, per, key, ticks=260, **over):
    """`per` perturbed inputs per plan around that plan's nominal closed loop (the oracle's: `ticks` ticks from the initial state, inputs
    from tick 20 on), counter-based draws."""
    from quadruped_gait_generation_ismpc_amd import workload
    tin = np.zeros(len(plans) * per, dtype=q.TICK_IN)
    for p, plan in enumerate(plans):
        outs, ins, _, _ = O.Oracle(oracle_params(O, N, **over), plan).rollout(O.initial_state(), 0, ticks)
        assert (outs["status"] & q.ST_ERROR_MASK).sum() == 0, f"plan {p}: the nominal closed loop carries an error bit"
        for j in range(per):
            u = np.random.Generator(np.random.Philox(key=key, counter=[0, 0, p, j])).random(7)
            r = tin[p * per + j:p * per + j + 1]
            r[:] = ins[20 + min(int(u[0] * (ticks - 20)), ticks - 21)].view(q.TICK_IN)
            pm = 2.0 * u - 1.0
            r["com_pos"][0, :2] += workload.PERTURB["pos_xy"] * pm[1:3]; r["com_vel"][0, :2] += workload.PERTURB["vel_xy"] * pm[3:5]
            r["com_pos"][0, 2] += workload.PERTURB["pos_z"] * pm[5]; r["com_vel"][0, 2] += workload.PERTURB["vel_z"] * pm[6]
    tin["reserved"] = q.pack_reserved(0, np.arange(len(tin)) // per)
    return tin


@pytest.fixture(scope="module")
def world(q):
    """The plans, the 192 inputs and the oracles' records of them (computed once, never changed)."""
    from oracle import oracle as O
    from quadruped_gait_generation_ismpc_amd import workload
    params = q.default_params(N=100)
    plans = workload.make_plans(P, params)
    tin = nominal_inputs(q, O, 100, plans, PER, workload.SEED + 104729)
    refs = {}

    def ref(z_hi=None):
        if z_hi not in refs:
            over = {} if z_hi is None else dict(z_ineq_hi=z_hi)
            r = np.concatenate([O.Oracle(oracle_params(O, 100, **over), plans[p]).solve(tin[p * PER:(p + 1) * PER])[0] for p in range(P)])
            r.setflags(write=False)
            refs[z_hi] = r
        return refs[z_hi]
    tin.setflags(write=False)
    return dict(params=params, plans=plans, tin=tin, ref=ref)


def compare(q, out, ref, mass=50.0, what=""):
    """The project's tolerances on the instances without an error bit on either side; returns that mask."""
    ok = ((ref["status"] | out["status"]) & q.ST_ERROR_MASK) == 0
    print(f"{what}: compared {ok.sum()} of {len(ok)}, status 0 on {(ref['status'][ok] == 0).sum()}")
    assert ok.mean() >= 0.9, (what, ok.mean())
    assert (ref["status"][ok] == 0).mean() >= 0.7, (what, (ref["status"][ok] == 0).mean())
    rel = np.abs(out["com_pos"] - ref["com_pos"]).max(1) / np.maximum(np.abs(ref["com_pos"]).max(1), 1e-3)
    print(f"{what}: CoM rel {rel[ok].max():.2e}, vel {np.abs(out['com_vel'] - ref['com_vel'])[ok].max():.2e}")
    assert rel[ok].max() <= TOL, (what, rel[ok].max())
    assert np.abs(out["com_vel"] - ref["com_vel"])[ok].max() <= TOL, what
    scale = np.maximum(np.array([9.81 * mass, 1.0, 1.0])[None, :], np.abs(ref["u0"][ok]))
    assert (np.abs(out["u0"] - ref["u0"])[ok] <= TOL * scale).all(), what
    assert (out["status"][ok] == ref["status"][ok]).all(), what
    return ok


def with_env(monkeypatch, make, **env):
    """make() under the given environment (None: unset); the handle reads its knobs when it is created."""
    for k, v in env.items():
        monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
    try:
        return make()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def expected_lanes(lay, batch):
    return int(lay) if lay else (32 if batch <= 2048 else 16 if batch <= 8192 else 8)


@pytest.mark.parametrize("lay", LAYOUTS)
def test_one_oracle_per_plan_in_every_layout(q, world, lay, monkeypatch):
    s = with_env(monkeypatch, lambda: q.MPCSolver.plans(world["plans"], world["params"]), ISMPC_LPI=lay)
    assert s.plans_info() == {"n_plans": P} and s.sweep_info()["n_sets"] == 1
    tin = world["tin"]
    out = s.solve_batch(tin)
    dev = q.from_device(s.solve_batch_torch(q.to_device(tin)), q.TICK_OUT)
    info = s.launch_info()
    assert (info["family"], info["lanes"], info["plans"], info["sweep"]) == ("quad_one", expected_lanes(lay, B), True, False), info
    assert out.tobytes() == dev.tobytes()
    # the other two host-buffer forms: the mapped staging block of batches <= 64, and page-locked caller records read and written in place
    assert s.solve_batch(tin[:40]).tobytes() == out[:40].tobytes()
    pin_in, pin_out = q.PinnedRecords(B, q.TICK_IN), q.PinnedRecords(B, q.TICK_OUT)
    pin_in.array[:] = tin
    s.reserve(B)
    assert s.solve_batch(pin_in.array, out=pin_out.array).tobytes() == out.tobytes()
    assert (out["status"] & q.ST_BAD_INDEX).sum() == 0
    compare(q, out, world["ref"](), what=f"lpi {lay}")
    for p in range(P):                                                     # the handle's plans are the ones it was given
        assert np.array_equal(s.midpoint(p)[:, :2], O_midpoint(world["plans"][p])[:, :2])
    assert np.array_equal(s.midpoint(), s.midpoint(0))
    # the plans matter: the same records with the plan index rotated by one
    t2 = tin.copy(); t2["reserved"] = q.pack_reserved(0, (np.arange(B) // PER + 1) % P)
    o2 = s.solve_batch(t2)
    both = (out["status"] == 0) & (o2["status"] == 0)
    moved = np.abs(out["u0"][:, 1:] - o2["u0"][:, 1:]).max(1)
    print(f"rotated plans: {both.sum()} instances with status 0 under both, min max(|du0_x|, |du0_y|) = {moved[both].min():.2e}")
    assert both.sum() >= 10 and (moved[both] > 1e-3).all()
    s.close()


def O_midpoint(plan):
    from oracle import oracle as O
    return O.Oracle(O.default_params(100), plan).midpoint()


@pytest.mark.parametrize("lay", LAYOUTS)
def test_records_are_bytewise_those_of_a_plain_handle_on_the_plan(q, world, lay, monkeypatch):
    import torch
    tin, N = world["tin"], 100
    s = with_env(monkeypatch, lambda: q.MPCSolver.plans(world["plans"], world["params"]), ISMPC_LPI=lay)
    d_in = q.to_device(tin)
    ut = torch.zeros((B, 3, N), dtype=torch.float64, device="cuda:0")
    out = s.solve_batch_torch(d_in, u_traj=ut)
    torch.cuda.synchronize()
    assert s.launch_info()["plans"]
    for p in range(P):
        plain = with_env(monkeypatch, lambda: q.MPCSolver(world["plans"][p], params=world["params"]), ISMPC_LPI=lay)
        mine = tin[p * PER:(p + 1) * PER].copy(); mine["reserved"] = 0
        up = torch.zeros((PER, 3, N), dtype=torch.float64, device="cuda:0")
        op = plain.solve_batch_torch(q.to_device(mine), u_traj=up)
        torch.cuda.synchronize()
        assert plain.launch_info()["lanes"] == s.launch_info()["lanes"] and "plans" not in plain.launch_info()
        assert plain.plans_info() == {"n_plans": 1}
        assert torch.equal(op, out[p * PER:(p + 1) * PER]), (lay, p)
        assert torch.equal(up, ut[p * PER:(p + 1) * PER]), (lay, p)
        assert up.abs().max() > 0
        plain.close()
    s.close()


def test_fallback_forms_agree_bytewise_and_with_the_oracles(q, world, monkeypatch):
    """z_ineq_hi = 4.6 makes the vertical inequality rows active on most of the sample: the two-launch form (ISMPC_ONE_LAUNCH=0: tick kernel,
    deferred list, fallback launch) and the one-launch form (3: ismpc_tick_quad_one calls the fallback itself) run it on the instance's own
    (set, plan) record."""
    p46 = q.default_params(N=100, z_ineq_hi=4.6)
    tin, outs = world["tin"], {}
    for form, family in (("0", "quad"), ("3", "quad_one")):
        s = with_env(monkeypatch, lambda: q.MPCSolver.plans(world["plans"], p46), ISMPC_ONE_LAUNCH=form)
        outs[form] = s.solve_batch(tin)
        info = s.launch_info()
        assert (info["family"], info["plans"], info["kernels"]) == (family, True, 2 if form == "0" else 1), info
        assert s.fallback_counters() == (0, 0, 0, 0)
        s.close()
    assert outs["0"].tobytes() == outs["3"].tobytes()
    ref = world["ref"](4.6)
    act = (ref["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    print(f"active vertical rows on {act.sum()} of {B}")
    assert act.mean() >= 0.6
    ok = ((ref["status"] | outs["0"]["status"]) & q.ST_ERROR_MASK) == 0
    assert ok.mean() >= 0.9
    # (with the vertical rows active the share of status 0 is the share of instances WITHOUT them: the horizontal stage ran wherever no
    # flight bit is set)
    assert ((ref["status"][ok] & ~q.ST_Z_INEQ_ACTIVE) == 0).mean() >= 0.7
    rel = np.abs(outs["0"]["com_pos"] - ref["com_pos"]).max(1) / np.maximum(np.abs(ref["com_pos"]).max(1), 1e-3)
    assert rel[ok].max() <= TOL and np.abs(outs["0"]["com_vel"] - ref["com_vel"])[ok].max() <= TOL
    scale = np.maximum(np.array([9.81 * 50.0, 1.0, 1.0])[None, :], np.abs(ref["u0"][ok]))
    assert (np.abs(outs["0"]["u0"] - ref["u0"])[ok] <= TOL * scale).all()
    assert (outs["0"]["status"][ok] == ref["status"][ok]).all() and ((outs["0"]["status"] & q.ST_Z_FAILED) == 0).all()


def test_what_ships_beyond_8192_instances(q, world, monkeypatch):
    import torch
    tin = world["tin"]
    s8 = with_env(monkeypatch, lambda: q.MPCSolver.plans(world["plans"], world["params"]), ISMPC_LPI="8")
    want = s8.solve_batch(tin).tobytes()
    s8.close()
    tiles = 44
    big = np.tile(tin, tiles)
    assert len(big) == 8448
    s = q.MPCSolver.plans(world["plans"], world["params"])
    d_in = q.to_device(big)
    got = s.solve_batch_torch(d_in).clone()
    info = s.launch_info()
    assert (info["family"], info["lanes"], info["plans"], info["kernels"], info["bound_order"]) == ("quad_one", 8, True, 1, False), info
    rec = q.from_device(got, q.TICK_OUT)
    for k in range(tiles):
        assert rec[k * B:(k + 1) * B].tobytes() == want, k
    s.sweep_bind(d_in)                                                     # placement only: sorted by (set, plan) pair
    again = s.solve_batch_torch(d_in)
    torch.cuda.synchronize()
    assert s.launch_info()["bound_order"] and torch.equal(again, got)
    s.close()


def test_sets_times_plans(q, world):
    from oracle import oracle as O
    from quadruped_gait_generation_ismpc_amd import workload
    K = 4
    sets = workload.make_sweep_params(K, N=100)
    s = q.MPCSolver.plans(world["plans"], sets)
    assert s.plans_info() == {"n_plans": P} and s.sweep_info()["n_sets"] == K
    tin = world["tin"].copy()
    kset = np.arange(B) % K
    tin["reserved"] = q.pack_reserved(kset, np.arange(B) // PER)
    out = s.solve_batch(tin)
    info = s.launch_info()
    assert info["plans"] and info["sweep"] and info["lanes"] == 16, info
    assert (out["status"] & q.ST_BAD_INDEX).sum() == 0
    ref = np.zeros(B, dtype=out.dtype)
    for k in range(K):
        for p in range(P):
            m = np.where((kset == k) & (np.arange(B) // PER == p))[0]
            ref[m] = O.Oracle(oracle_params(O, 100, sets[k]), world["plans"][p]).solve(tin[m])[0]
    # (one tolerance scale for u0_z over the sets: the lightest set's weight, the tightest)
    compare(q, out, ref, mass=min(p.mass for p in sets), what="sets x plans")
    for p in (1, 6):                                                       # ... and the sweep handle built on that plan alone
        sw = q.MPCSolver.sweep(world["plans"][p], sets)
        mine = tin[p * PER:(p + 1) * PER].copy(); mine["reserved"] = kset[p * PER:(p + 1) * PER]
        a, b = sw.solve_batch(mine), out[p * PER:(p + 1) * PER]
        assert np.array_equal(a["status"], b["status"])
        assert np.abs(a["com_pos"] - b["com_pos"]).max() <= 1e-9 and np.abs(a["com_vel"] - b["com_vel"]).max() <= 1e-9
        assert (np.abs(a["u0"] - b["u0"]) <= 1e-9 * np.maximum(np.abs(a["u0"]), 1.0)).all()
        sw.close()
    bad = tin[:6].copy()
    bad["reserved"] = [q.pack_reserved(0, 8), q.pack_reserved(4, 0), -1, q.pack_reserved(3, 7), q.pack_reserved(4, 8), q.pack_reserved(0, 0)]
    ob = s.solve_batch(bad)
    flagged = (ob["status"] & q.ST_BAD_INDEX) != 0
    assert flagged.tolist() == [True, True, True, False, True, False]
    assert np.array_equal(ob["com_pos"][flagged], bad["com_pos"][flagged]) and np.array_equal(ob["com_vel"][flagged], bad["com_vel"][flagged])
    s.close()


def test_closed_loop_with_per_plan_step_timing(q, world, monkeypatch):
    """The in-kernel rollout against one launch per tick, byte for byte, and against each plan's oracle: plans with T = 40 frames step at
    ticks 39, 79 and 119, those with T = 45 at 44 and 89 -- a kernel that read plan 0's timings would count other footsteps."""
    import torch
    from oracle import oracle as O
    plans, ticks = world["plans"], 130
    a = with_env(monkeypatch, lambda: q.MPCSolver.plans(plans, world["params"]), ISMPC_ROLLOUT=None)
    b = with_env(monkeypatch, lambda: q.MPCSolver.plans(plans, world["params"]), ISMPC_ROLLOUT="host")
    recs = np.repeat(O.initial_state().view(q.TICK_IN), 2 * P)
    rng = np.random.default_rng(9)
    recs["com_pos"][1::2, :2] += rng.uniform(-0.004, 0.004, (P, 2)); recs["com_vel"][1::2, :2] += rng.uniform(-0.02, 0.02, (P, 2))
    recs["reserved"] = q.pack_reserved(0, np.arange(2 * P) // 2)
    sa, sb = q.to_device(recs), q.to_device(recs)
    ta = a.rollout_torch(sa, 0, ticks); tb = b.rollout_torch(sb, 0, ticks)
    torch.cuda.synchronize()
    ia, ib = a.launch_info(), b.launch_info()
    assert ia["family"] == "rollout_quad" and ia["plans"] and ib["family"] != "rollout_quad" and ib["plans"], (ia, ib)
    assert torch.equal(ta, tb) and torch.equal(sa, sb)
    out, endst = q.from_device(ta, q.TICK_OUT), q.from_device(sa, q.TICK_IN)
    counters = set()
    for p in range(P):
        ref, ins, _, fin = O.Oracle(O.default_params(100), plans[p]).rollout(O.initial_state(), 0, ticks)
        T = int(plans[p][1, 3])
        steps = np.where(np.diff(ins["footstep_counter"]) == 1)[0] + 1     # ticks at which the oracle's bookkeeping moved to the next footstep
        assert len(steps) >= 2 and (np.diff(steps) == T).all(), (p, T, steps)
        o = out[:, 2 * p]
        assert (ref["status"] & q.ST_ERROR_MASK).sum() == 0 and np.array_equal(o["status"], ref["status"]), p
        rel = np.abs(o["com_pos"] - ref["com_pos"]).max(1) / np.maximum(np.abs(ref["com_pos"]).max(1), 1e-3)
        assert rel.max() <= TOL and np.abs(o["com_vel"] - ref["com_vel"]).max() <= TOL, (p, rel.max())
        scale = np.maximum(np.array([9.81 * 50.0, 1.0, 1.0])[None, :], np.abs(ref["u0"]))
        assert (np.abs(o["u0"] - ref["u0"]) <= TOL * scale).all(), p
        for k in ("mpc_iter", "control_iter", "footstep_counter", "simulation_time"):
            assert endst[k][2 * p] == fin[k][0], (p, k)
        assert endst["reserved"][2 * p] == q.pack_reserved(0, p)
        counters.add((int(fin["footstep_counter"][0]), int(fin["mpc_iter"][0])))
    assert len(counters) >= 2                                              # the plans do step at different ticks
    a.close(); b.close()


def test_one_instance_per_wavefront_at_N150(q):
    from oracle import oracle as O
    from quadruped_gait_generation_ismpc_amd import workload
    N, NP, per = 150, 4, 6
    params = q.default_params(N=N)
    plans = workload.make_plans(NP, params)
    tin = nominal_inputs(q, O, N, plans, per, workload.SEED + 104729 + N, ticks=140)     # (three footsteps of every plan; the oracle is slow at this horizon)
    s = q.MPCSolver.plans(plans, params)
    out = s.solve_batch(tin)
    info = s.launch_info()
    assert (info["family"], info["plans"]) == ("affine", True), info
    ref = np.concatenate([O.Oracle(O.default_params(N), plans[p]).solve(tin[p * per:(p + 1) * per])[0] for p in range(NP)])
    compare(q, out, ref, what="N = 150")
    bad = tin[:2].copy(); bad["reserved"] = [q.pack_reserved(0, NP), q.pack_reserved(1, 0)]
    ob = s.solve_batch(bad)
    assert ((ob["status"] & q.ST_BAD_INDEX) != 0).all() and np.array_equal(ob["com_pos"], bad["com_pos"])
    s.close()


def test_plans_that_share_a_height_profile(q):
    """Footsteps off z = 0 (the "stairs" column of tests/test_gpu_parity.py::new_solver) on three x / y variants: one set of offset tables
    serves every plan."""
    from oracle import oracle as O
    from quadruped_gait_generation_ismpc_amd import workload
    params = q.default_params(N=100)
    plans = [f.copy() for f in workload.make_plans(3, params)]
    for f in plans:
        for i in range(1, f.shape[0]):
            f[i, 2] = 0.01 * ((i // 3) % 4)
    nominal = O.Oracle(O.default_params(100), plans[0]).rollout(O.initial_state(), 0, 260)[0]
    if (nominal["status"] & q.ST_ERROR_MASK).any():
        pytest.skip("the nominal closed loop on the stairs column carries error bits: no nominal states to perturb")
    per = 16
    tin = nominal_inputs(q, O, 100, plans, per, workload.SEED + 104729 + 1)
    s = q.MPCSolver.plans(plans, params)
    out = s.solve_batch(tin)
    assert s.launch_info()["plans"]
    ref = np.concatenate([O.Oracle(O.default_params(100), plans[p]).solve(tin[p * per:(p + 1) * per])[0] for p in range(3)])
    compare(q, out, ref, what="stairs")
    flat = np.concatenate([O.Oracle(O.default_params(100), workload.make_plans(3, params)[p]).solve(tin[p * per:(p + 1) * per])[0] for p in range(3)])
    assert np.abs(ref["u0"][:, 0] - flat["u0"][:, 0]).max() > 1.0           # the heights do matter
    s.close()
