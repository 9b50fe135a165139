"""Every kernel form launch() dispatches for Formulation B, against the CPU oracle AT THE BATCH SIZE WHERE IT RUNS.

The lane-group kernels are picked by batch size (csrc/ismpc_hip.hip: 32 / 16 / 8 lanes per instance; ismpc_tick_quad_inline while every
wavefront is resident, ismpc_tick_quad_one or ismpc_tick_quad + ismpc_tick_affine_fallback beyond; ismpc_rollout_quad for closed loops;
the SW instantiations for sweep handles).  The arithmetic template is shared, so what a small batch cannot see is the dispatch itself, the
ragged tail, the occupancy-dependent register allocation of each instantiation and the deferred paths at full grid size.  Every test here
first asserts MPCSolver.launch_info() -- which kernel the step took, written down from the dispatch RULE, not read back -- and only then
compares a fixed sample of the batch with the oracle (reference qpOASES where oracle/_ref is built).

Tolerances are the project's own: TOL = 1e-6 and assert_parity of test_gpu_parity; a status may differ from the oracle's only in the
infeasibility bits of a horizontal QP within 1e-9 (relative) of its feasibility boundary.
"""
import contextlib
import os

import numpy as np
import pytest

from test_gpu_parity import TOL, assert_parity, rel_com, _on_feasibility_boundary

pytestmark = pytest.mark.gpu

BATCH = 20001                # odd: ragged for every layout; beyond the resident size of all three on a 256-CU part (asserted from the rule)
ENV_KEYS = ("ISMPC_PATH", "ISMPC_LPI", "ISMPC_ROLLOUT", "ISMPC_ONE_LAUNCH")
FORMS = {"one": "3", "two": "0"}          # ISMPC_ONE_LAUNCH
# the shape table of launch() restated: (lanes per instance, N) -> (R, RW).  Every instantiated quad_shape row appears once.
SHAPES = {(8, 50): (8, 1), (8, 100): (13, 2), (8, 128): (16, 2),
          (16, 50): (4, 1), (16, 100): (7, 2), (16, 128): (8, 2),
          (32, 50): (4, 1), (32, 100): (4, 2),
          (8, 37): (8, 1)}                 # N = 37 = 4 * 8 + 5: the last sample row of a lane group is masked beyond five lanes
MATRIX = sorted(SHAPES)


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


@pytest.fixture(scope="module")
def cus(q):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- the dispatch rule, written down independently of the library ---------------------------------------------------------------------
def expected_step(cus, batch, N, lpi=None, one_launch=None, sweep=False, bound=False):
    """What launch_info() must report for one ismpc_solve_batch* step of a FRESH handle (no deferral seen yet): lanes by batch size unless
    ISMPC_LPI fixes them (sweep handles: 16, 8 beyond 8 192), resident while waves <= 8 * CUs, then the form by ISMPC_ONE_LAUNCH."""
    if lpi is None:
        lpi = (8 if batch > 8192 else 16) if sweep else (32 if batch <= 2048 else 16 if batch <= 8192 else 8)
    waves = (batch * lpi + 63) // 64
    resident = waves <= 8 * cus
    if one_launch == 0:
        family, kernels = "quad", 2
    elif resident and not sweep:
        family, kernels = "quad_inline", 1
    else:
        family, kernels = "quad_one", 1
    need = -(-N // lpi)
    R = {32: 4, 16: 4 if need <= 4 else 7 if need <= 7 else 8, 8: 8 if need <= 8 else 13 if need <= 13 else 16}[lpi]
    return {"family": family, "lanes": lpi, "R": R, "RW": 1 if N <= 64 else 2, "sweep": sweep, "kernels": kernels, "batch": batch,
            "bound_order": bound}


@contextlib.contextmanager
def knobs(**env):
    """The run-time knobs a handle reads at creation, set as solver_for sets them: saved, cleared, set, restored."""
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items() if v is not None})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def fresh_solver(q, N, lpi=None, form=None, sets=None):
    p = q.default_params(N=N)
    with knobs(ISMPC_PATH="affine", ISMPC_LPI=lpi, ISMPC_ONE_LAUNCH=FORMS.get(form)):
        if sets is not None:
            return q.MPCSolver.sweep(q.reference_plan(params=sets[0]), sets)
        return q.MPCSolver(q.reference_plan(params=p), params=p)


# ---- inputs, samples, the comparison ---------------------------------------------------------------------------------------------------
def lift(tin, N, every=4):
    """Every instance with i % 4 == 1 starts far above h_des with an upward velocity: its first vertical forces hit the lower bound of
    0 <= S_bar_z u (MPCSolver.cpp:158-160), so the tick kernel defers it.  With the oracle alone (1 536 instances per horizon, N = 50, 64,
    100, 128): every lifted instance is ST_Z_INEQ_ACTIVE, no other one is, none of them is in error -- every wavefront of every layout
    holds deferred and non-deferred instances side by side."""
    sel = np.arange(len(tin)) % every == 1
    tin["com_pos"][sel, 2] += 0.25 if N >= 100 else 0.12
    tin["com_vel"][sel, 2] += 0.2
    return sel


def matrix_batch(N, batch=BATCH):
    from quadruped_gait_generation_ismpc_amd import workload
    base = 200 if N > 150 else (100 if N > 50 else 50)                  # as test_against_oracle_seeded picks it
    tin = workload.make_batch(base, batch, seed=4000 + N)
    lift(tin, N)
    return tin


def sample_indices(batch, n, seed):
    """The first 8, the last 8 (the ragged tail) and n - 16 drawn with a fixed seed: fixed before the device runs."""
    mid = 8 + np.random.default_rng(seed).choice(batch - 16, n - 16, replace=False)
    return np.concatenate([np.arange(8), np.sort(mid), np.arange(batch - 8, batch)])


def compare_with_oracle(q, out, ref, boundary):
    """The comparison every test of this file applies to a sample: `out` (device) against `ref` (oracle), same order.
      * ST_Z_INEQ_ACTIVE equal on every instance;
      * a status differs only in ST_X/Y_INFEASIBLE, and only where boundary(i) says the QP is within 1e-9 of its feasibility boundary;
      * assert_parity (CoM, CoM velocity, u0 within TOL; status equal) over the instances neither side flags as in error;
      * the fallback reports at least one iteration on every active instance.
    Returns the mask of the instances that went through assert_parity."""
    act = (ref["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    got = (out["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    assert (got == act).all(), np.flatnonzero(got != act)
    for i in np.flatnonzero(out["status"] != ref["status"]):
        assert ((int(out["status"][i]) ^ int(ref["status"][i])) & ~(q.ST_X_INFEASIBLE | q.ST_Y_INFEASIBLE)) == 0, (i, out["status"][i], ref["status"][i])
        assert boundary(i), (i, out["status"][i], ref["status"][i])
    ok = ((ref["status"] | out["status"]) & q.ST_ERROR_MASK) == 0
    assert_parity(q, out, ref, ok)
    if (act & ok).any():
        assert ((out["iters"][act & ok] >> 16) & 255).min() >= 1
    return ok


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def matrix_case(O, N):
    """Inputs of horizon N, the fixed sample and the oracle's records of it (solved once, reused by every form of the horizon)."""
    def make():
        tin = matrix_batch(N)
        pick = sample_indices(BATCH, 96, seed=N)
        ref, _ = O.Oracle(O.default_params(N)).solve(tin[pick])
        return tin, pick, ref
    return cached(("matrix", N), make)


def check_sample_conditions(q, ref, n_active, n_inactive, feasible):
    act = (ref["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    good = (ref["status"] & q.ST_ERROR_MASK) == 0
    print(f"sample: {len(ref)} instances, active {int(act.sum())}, inactive {int((~act).sum())}, oracle-feasible {int(good.sum())}")
    assert act.sum() >= n_active and (~act).sum() >= n_inactive and good.mean() >= feasible, (act.sum(), (~act).sum(), good.mean())
    return act


def run_form(q, lanes, N, form, tin):
    """One step of a fresh handle forced to `lanes` lanes per instance in the one- or the two-launch form: (records, launch_info)."""
    def make():
        s = fresh_solver(q, N, lpi=lanes, form=form)
        try:
            out = s.solve_batch(tin)
            return out, s.launch_info()
        finally:
            s.close()
    return cached(("form", lanes, N, form), make)


# ---- form x shape matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "two"])
@pytest.mark.parametrize("lanes,N", MATRIX)
def test_form_and_shape_against_oracle_at_size(q, O, cus, lanes, N, form):
    """ismpc_tick_quad_one<R, LPI, RW, false> (its fallback_call_one at the instantiation's own one_occ) and ismpc_tick_quad<R, LPI> +
    the deferred list + ismpc_tick_affine_fallback at full grid size, one id per instantiated shape and form: 20 001 instances, a quarter
    of them deferred, 96 of them (ragged tail included) against the oracle."""
    tin, pick, ref = matrix_case(O, N)
    out, info = run_form(q, lanes, N, form, tin)
    want = expected_step(cus, BATCH, N, lpi=lanes, one_launch=int(FORMS[form]))
    print(f"launch_info[{lanes}-{N}-{form}] = {info}")
    assert (BATCH * lanes + 63) // 64 > 8 * cus                      # beyond the resident size: not the inline kernel
    assert want["family"] == ("quad_one" if form == "one" else "quad") and (want["R"], want["RW"]) == SHAPES[(lanes, N)]
    assert info == want
    act = check_sample_conditions(q, ref, n_active=16, n_inactive=48, feasible=0.8)
    assert ((out["status"] & q.ST_Z_FAILED) == 0).all()
    assert (((out["status"] & q.ST_Z_INEQ_ACTIVE) != 0).mean() > 0.2)            # the deferred paths do run at grid size
    compare_with_oracle(q, out[pick], ref, lambda i: _on_feasibility_boundary(q, N, tin[pick[i]], band=1e-9))
    assert act.any()


@pytest.mark.parametrize("lanes,N", MATRIX)
def test_one_launch_and_two_launch_records_are_byte_equal_per_shape(q, O, cus, lanes, N):
    tin, _, _ = matrix_case(O, N)
    a, ia = run_form(q, lanes, N, "one", tin)
    b, ib = run_form(q, lanes, N, "two", tin)
    assert (ia["family"], ia["kernels"], ib["family"], ib["kernels"]) == ("quad_one", 1, "quad", 2)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N", [50, 100, 128])
def test_default_dispatch_prefix_is_bytewise_the_small_forced_launch(q, O, cus, N):
    """Ties the small-batch tests (the inline kernel) to the large-batch forms: the first 2 000 records of the default-dispatch 20 001
    batch (8 lanes per instance, ismpc_tick_quad_one) equal, byte for byte, a 2 000-instance launch forced to the same layout, which is
    resident and takes ismpc_tick_quad_inline."""
    tin, _, _ = matrix_case(O, N)
    big = fresh_solver(q, N)
    small = fresh_solver(q, N, lpi=8)
    try:
        a = big.solve_batch(tin)
        ia = big.launch_info()
        b = small.solve_batch(tin[:2000])
        ib = small.launch_info()
    finally:
        big.close(); small.close()
    print(f"launch_info[default-{N}] = {ia}; [lpi8-2000] = {ib}")
    assert ia == expected_step(cus, BATCH, N) and (ia["family"], ia["lanes"]) == ("quad_one", 8)
    assert ib == expected_step(cus, 2000, N, lpi=8) and ib["family"] == "quad_inline"
    assert (((b["status"] & q.ST_Z_INEQ_ACTIVE) != 0).sum() >= 400)
    assert a[:2000].tobytes() == b.tobytes()
    forced, _ = run_form(q, 8, N, "one", tin)
    assert a.tobytes() == forced.tobytes()


# ---- heavy regime at size --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [65536, 20001])
def test_heavy_regime_at_size(q, O, cus, batch):
    """scale = 2.0: infeasible horizontal QPs and many clipped samples in the knapsack Newton, in the kernel the default dispatch takes at
    this size (ismpc_tick_quad_one<13, 8, 2, false>), 192 sampled instances against the oracle."""
    from quadruped_gait_generation_ismpc_amd import workload
    N = 100
    tin = workload.make_batch(N, batch, scale=2.0, seed=4200)
    pick = sample_indices(batch, 192, seed=batch)
    ref, _ = O.Oracle(O.default_params(N)).solve(tin[pick])
    s = fresh_solver(q, N)
    try:
        out = s.solve_batch(tin)
        info = s.launch_info()
    finally:
        s.close()
    print(f"launch_info[heavy-{batch}] = {info}")
    assert info == expected_step(cus, batch, N) and (info["family"], info["lanes"], info["R"], info["RW"]) == ("quad_one", 8, 13, 2)
    good = (ref["status"] & q.ST_ERROR_MASK) == 0
    infeasible = (ref["status"] & (q.ST_X_INFEASIBLE | q.ST_Y_INFEASIBLE)) != 0
    print(f"sample: 192 instances, oracle-feasible {int(good.sum())}, X- or Y-infeasible {int(infeasible.sum())}")
    assert good.mean() >= 0.5 and infeasible.sum() >= 20, (good.mean(), infeasible.sum())
    assert ((out["status"] & q.ST_Z_FAILED) == 0).all()
    compare_with_oracle(q, out[pick], ref, lambda i: _on_feasibility_boundary(q, N, tin[pick[i]], band=1e-9))


# ---- sweep instantiations --------------------------------------------------------------------------------------------------------------
def _set_over(p):
    return dict(mass=p.mass, h_des=p.h_des, q_p=p.q_p, q_u=p.q_u, q_v=p.q_v, foot_width=p.foot_width)


def sweep_case(q, O):
    """8 parameter sets, 20 001 instances (set i % 8), 12 sampled instances of each set -- its first, its last and 10 drawn with a fixed
    seed -- and one oracle per set.  The lift is the matrix's (i % 4 == 1), kept as it is there: with the set taken as i % 8 it puts every
    instance of sets 1 and 5 among the deferred ones and none of the other six sets, so the fallback body meets the oracle under two
    parameter sets and the tick proper under six; each wavefront of the unbound launch still holds both kinds side by side, and a
    wavefront of the bound launch (one set per wavefront) holds only one.  (tests/test_gpu_sweep.py has the oracle on all 64 sets of
    its batch, small-batch kernels, with a tight z_ineq_hi in its fallback cases.)"""
    def make():
        from quadruped_gait_generation_ismpc_amd import workload
        sets = workload.make_sweep_params(8, N=100)
        tin = workload.make_batch(100, BATCH, seed=4300)
        lift(tin, 100)
        tin["reserved"] = np.arange(BATCH) % 8
        picks, refs = [], []
        for k in range(8):
            mine = np.flatnonzero(tin["reserved"] == k)
            pk = np.concatenate([mine[:1], np.sort(np.random.default_rng(k).choice(mine[1:-1], 10, replace=False)), mine[-1:]])
            ref, _ = O.Oracle(O.default_params(100, **_set_over(sets[k]))).solve(tin[pk])
            picks.append(pk); refs.append(ref)
        return sets, tin, picks, refs
    return cached("sweep", make)


def run_sweep(q, O, lanes, form, bound):
    """One step of a fresh sweep handle at `lanes` lanes per instance (16: ISMPC_LPI=16; 8: a sweep handle's default beyond 8 192) in the
    one- or the two-launch form, with or without the ismpc_sweep_bind order: (records, launch_info, fallback_counters)."""
    def make():
        import torch
        sets, tin, _, _ = sweep_case(q, O)
        d_in = q.to_device(tin)
        s = fresh_solver(q, 100, lpi=16 if lanes == 16 else None, form=form, sets=sets)
        try:
            if bound:
                s.sweep_bind(d_in)
            d_out = s.solve_batch_torch(d_in)
            torch.cuda.synchronize()
            return q.from_device(d_out, q.TICK_OUT), s.launch_info(), s.fallback_counters()
        finally:
            s.close()
    return cached(("sweep-run", lanes, form, bound), make)


@pytest.mark.parametrize("bound", [False, True], ids=["unbound", "bound"])
@pytest.mark.parametrize("form", ["one", "two"])
@pytest.mark.parametrize("lanes", [16, 8])
def test_sweep_instantiations_at_size(q, O, cus, lanes, form, bound):
    """ismpc_tick_quad_one<R, LPI, RW, true> and ismpc_tick_quad<R, LPI, true> + ismpc_tick_affine_fallback<2, true> at 16 lanes
    (ISMPC_LPI=16) and 8 lanes (a sweep handle's default beyond 8 192), with and without the ismpc_sweep_bind order."""
    sets, tin, picks, refs = sweep_case(q, O)
    out, info, counters = run_sweep(q, O, lanes, form, bound)
    print(f"launch_info[sweep-{lanes}-{form}-{'bound' if bound else 'unbound'}] = {info}")
    assert info == expected_step(cus, BATCH, 100, lpi=16 if lanes == 16 else None, one_launch=int(FORMS[form]), sweep=True, bound=bound)
    assert info["sweep"] and info["lanes"] == lanes and info["bound_order"] == bound
    assert counters == (0, 0, 0, 0)
    assert ((out["status"] & (q.ST_Z_FAILED | q.ST_BAD_INDEX)) == 0).all()
    n_act = n_ok = 0
    for k in range(8):
        over = _set_over(sets[k])

        def boundary(i, k=k, over=over):
            return _on_feasibility_boundary(q, 100, tin[picks[k][i]], band=1e-9, **over)
        ok = compare_with_oracle(q, out[picks[k]], refs[k], boundary)
        n_act += int(((refs[k]["status"] & q.ST_Z_INEQ_ACTIVE) != 0).sum()); n_ok += int(ok.sum())
    print(f"sample: 96 instances over 8 sets, active {n_act}, inactive {96 - n_act}, compared {n_ok}")
    assert n_act >= 16 and n_ok >= 72                       # (the oracle alone: 24 active, 95 feasible)


@pytest.mark.parametrize("lanes", [16, 8])
def test_sweep_records_are_byte_equal_across_forms_and_placement(q, O, lanes):
    """Per layout: one launch or two, bound order or not -- placement and launch form only, the same bytes."""
    ref, _, _ = run_sweep(q, O, lanes, "one", False)
    for form in ("one", "two"):
        for bound in (False, True):
            out, info, _ = run_sweep(q, O, lanes, form, bound)
            assert (info["family"], info["kernels"], info["bound_order"]) == (("quad_one", 1) if form == "one" else ("quad", 2)) + (bound,)
            assert out.tobytes() == ref.tobytes(), (form, bound)


# ---- closed loop at size ---------------------------------------------------------------------------------------------------------------
ROLL_B, ROLL_TICKS, ROLL_FRAME = 65536, 20, 400


def rollout_states(batch, lifted):
    """65 536 perturbed copies of the nominal closed loop's state at frame ROLL_FRAME (the committed pre-roll; perturbation half-widths
    of workload.PERTURB).  ismpc_rollout_device sets ONE simulationTime for the whole batch (Controller.cpp:310), so states whose footstep
    plan the oracle can follow for 20 ticks all stem from one frame: instances drawn from frames all over the gait (workload.make_batch)
    are infeasible from the first tick in the oracle itself, where qpOASES' returned point is not specified."""
    from quadruped_gait_generation_ismpc_amd import workload
    table, lo, hi = workload.load_preroll(100)
    st = np.repeat(table[ROLL_FRAME:ROLL_FRAME + 1], batch)
    assert st["simulation_time"][0] == ROLL_FRAME
    u = np.random.Generator(np.random.Philox(key=4400)).uniform(-1.0, 1.0, (batch, 6))
    P = workload.PERTURB
    st["com_pos"][:, :2] += P["pos_xy"] * u[:, 0:2]; st["com_vel"][:, :2] += P["vel_xy"] * u[:, 2:4]
    st["com_pos"][:, 2] += P["pos_z"] * u[:, 4]; st["com_vel"][:, 2] += P["vel_z"] * u[:, 5]
    if lifted:
        lift(st, 100)
    return st


def compare_rollout(q, out, refs, fin, ref_fin):
    """out: [ticks, n] device records; refs: n oracle trajectories.  Per instance: statuses equal and rel_com <= TOL on every tick up to
    the first one either side flags as in error (assert_parity's rule along the loop: past an infeasible horizontal QP the two sides feed
    different points back), counters bit exact on all.  Returns the number of instance-ticks compared."""
    n_cmp = 0
    for j, ref in enumerate(refs):
        o = out[:, j]
        err = ((o["status"] | ref["status"]) & q.ST_ERROR_MASK) != 0
        upto = int(err.argmax()) if err.any() else len(ref)
        assert np.array_equal(o["status"][:upto + 1], ref["status"][:upto + 1]), (j, o["status"], ref["status"])
        if upto:
            assert rel_com(o[:upto], ref[:upto]).max() <= TOL, (j, rel_com(o[:upto], ref[:upto]).max())
        n_cmp += upto
        for k in ("mpc_iter", "control_iter", "footstep_counter", "simulation_time"):
            assert fin[k][j] == ref_fin[j][k][0], (j, k)
    return n_cmp


@pytest.mark.parametrize("lifted", [False, True], ids=["nominal", "lifted"])
def test_closed_loop_at_size(q, O, cus, lifted):
    """ismpc_rollout_quad<7, 16, 2> at the size of the benchmark's sustained leg: 65 536 states, 20 ticks in one launch, 48 sampled
    instances (the last one included) against the oracle's closed loop of the same state and frame.  lifted: every fourth instance is
    parked by the first launch (active vertical inequality rows) and finished by the resume launch -- about 16 000 of them."""
    import torch
    st = rollout_states(ROLL_B, lifted)
    frame = int(st["simulation_time"].max()) + 1                      # the convention of test_one_launch_and_two_launch_forms_agree_bitwise
    pick = np.concatenate([np.arange(4), np.sort(4 + np.random.default_rng(48).choice(ROLL_B - 8, 40, replace=False)), np.arange(ROLL_B - 4, ROLL_B)])
    orc = O.Oracle(O.default_params(100))
    refs, ref_fin = [], []
    for i in pick:
        r, _, _, f = orc.rollout(st[i:i + 1], frame, ROLL_TICKS)
        refs.append(r); ref_fin.append(f)
    ref_act = np.array([((r["status"] & q.ST_Z_INEQ_ACTIVE) != 0).any() for r in refs])
    clean = sum(int((((r["status"] & q.ST_ERROR_MASK) != 0).argmax()) if ((r["status"] & q.ST_ERROR_MASK) != 0).any() else ROLL_TICKS) for r in refs)
    print(f"sample: 48 instances, {int(ref_act.sum())} with active rows in the oracle's loop, oracle error-free instance-ticks {clean} of {48 * ROLL_TICKS}")
    assert clean == 48 * ROLL_TICKS if not lifted else clean >= 0.75 * 48 * ROLL_TICKS      # (the oracle alone: 938 of 960 lifted, 960 nominal)
    assert (ref_act.sum() >= 8) if lifted else (ref_act.sum() == 0)
    s = fresh_solver(q, 100)
    try:
        d_state = q.to_device(st)
        traj = s.rollout_torch(d_state, frame, ROLL_TICKS)
        torch.cuda.synchronize()
        info = s.launch_info()
        counters = s.fallback_counters()
        out = q.from_device(traj[:, torch.as_tensor(pick, device=traj.device)], q.TICK_OUT)
        status = q.from_device(traj, q.TICK_OUT)["status"]
        fin = q.from_device(d_state, q.TICK_IN)[pick]
    finally:
        s.close()
    print(f"launch_info[rollout-{'lifted' if lifted else 'nominal'}] = {info}")
    assert info == {"family": "rollout_quad", "lanes": 16, "R": 7, "RW": 2, "sweep": False, "kernels": 2, "batch": ROLL_B, "bound_order": False}
    assert counters == (0, 0, 0, 0)
    assert ((status & q.ST_Z_FAILED) == 0).all()
    parked = ((status & q.ST_Z_INEQ_ACTIVE) != 0).any(axis=0)
    print(f"instances that went through the resume launch: {int(parked.sum())}")
    if lifted:
        assert parked.sum() >= 16000                                  # (16 384 lifted instances)
    n_cmp = compare_rollout(q, out, refs, fin, ref_fin)
    print(f"instance-ticks compared: {n_cmp}")
    # nominal: the oracle's loop is error-free on every sampled instance, so every tick of all 48 is compared
    assert n_cmp == 48 * ROLL_TICKS if not lifted else n_cmp >= 0.75 * 48 * ROLL_TICKS
