"""Formulation B kernels at the horizon edges of every shape, against the CPU oracle.

Every kernel shape pads the horizon N up to lanes x R samples (lane-group kernels), 64 x ceil(N / 64) (one instance per wavefront, dense,
the vertical fallback) or a 64 / 128 / 256 GEMM tile (the sweep's table build), and masks the samples n >= N in the suffix scan, the
knapsack counts, the most-violated-row search of the fallback, the equality patterns, the u_traj stores (3 N doubles per instance, no
slack) and the identity padding of the Hessian tiles.  A mask that is off by one sample is invisible in the middle of a shape and wrong
next to a switch, so the horizons here are named by what changes there (HORIZONS below, written down from the dispatch RULE, not read
back from the library): both sides of every R / RW switch, N below the lane count (whole lanes own no sample), one live lane in the
second sample row, and N = 1, 2 where the scan has nothing to scan.

Inputs are 64 instances per horizon, built and checked from the oracle alone before the device runs (edge_case): below N = 57 the gait
generator of workload.make_batch is infeasible in the oracle itself (it draws states of the N = 50 gait), so the states come from the
oracle's own closed loop at horizon N; from 57 up they are the generator's.  The odd instances are lifted above h_des with an upward
velocity, so the vertical inequality rows are active on them (the fallback runs) wherever the horizon is long enough for that.

Tolerances are the project's own: TOL = 1e-6 and assert_parity of test_gpu_parity, statuses by the rule of test_against_oracle_seeded,
trajectories by the bounds of test_decision_trajectories.
"""
import contextlib
import os

import numpy as np
import pytest

from test_gpu_parity import TOL, assert_parity, rel_com, _on_feasibility_boundary

pytestmark = pytest.mark.gpu

B = 64
SEED0 = 5100               # inputs of horizon N are drawn with seed SEED0 + N ...
SEED_OF = {33: 33}         # ... but for 33: with 5133 no horizontal QP of the batch changes its working set (the oracle alone)
# ---- the edge matrix --------------------------------------------------------------------------------------------------------------------
# every layout: 7 < one sample row at 8 lanes; 9 / 17 / 33 = one live lane in the second row at 8 / 16 / 32 lanes (and N < lanes for the
# wider layouts); 1, 2: degenerate (one sample, one scan step)
COMMON = (1, 2, 7, 8, 9, 17, 33)
HORIZONS = {
    "lpi8": COMMON + (63, 64, 65, 104, 105, 128),          # 8 lanes: R = 8 | 13 at 64 | 65, 13 | 16 at 104 | 105, 128 = the last sample of R = 16
    "affine": COMMON + (63, 64, 65, 112, 113, 128),        # 16 lanes: R = 4 | 7 at 64 | 65, 7 | 8 at 112 | 113
    "lpi32": COMMON + (64, 65, 127, 128),                  # 32 lanes: R = 4 throughout, RW = 1 | 2 at 64 | 65; 127 / 128 = the last lane's last sample
    "wave": COMMON + (64, 65, 128, 129, 192, 193, 255, 256),     # one instance per wavefront: R = ceil(N / 64) = 1 | 2 | 3 | 4
    "dense": COMMON + (64, 65, 128, 129, 192, 193, 255, 256),
    "auto": COMMON + (129, 256),                           # default dispatch: 32 lanes at this batch size up to N = 128, ismpc_tick_affine beyond
}
PAIRS = [(lay, N) for lay in ("affine", "lpi8", "lpi32", "auto", "wave", "dense") for N in HORIZONS[lay]]
LANES = {"affine": 16, "lpi8": 8, "lpi32": 32, "auto": 32}
ENV = {"affine": {"ISMPC_PATH": "affine", "ISMPC_LPI": "16"}, "lpi8": {"ISMPC_PATH": "affine", "ISMPC_LPI": "8"},
       "lpi32": {"ISMPC_PATH": "affine", "ISMPC_LPI": "32"}, "auto": {"ISMPC_PATH": "affine"},
       "wave": {"ISMPC_PATH": "wave"}, "dense": {"ISMPC_PATH": "dense"}}
ENV_KEYS = ("ISMPC_PATH", "ISMPC_LPI", "ISMPC_ROLLOUT", "ISMPC_ONE_LAUNCH", "ISMPC_Z_LDS_Q", "ISMPC_Z_FALLBACK", "ISMPC_WAVES")


def quad_rule(lanes, N):
    """(R, RW) of the lane-group kernels: the smallest instantiated samples-per-lane that covers N; RW = ceil(N / 64) of the fallback body."""
    need = -(-N // lanes)
    R = {32: 4, 16: 4 if need <= 4 else 7 if need <= 7 else 8, 8: 8 if need <= 8 else 13 if need <= 13 else 16}[lanes]
    assert lanes * R >= N
    return R, (1 if N <= 64 else 2)


def expected_shape(lay, N, form=None):
    """(family, lanes, R, RW, kernels) launch_info() must report for one 64-instance step of layout `lay`: 64 instances are resident at
    every lane count, so a lane-group handle takes ismpc_tick_quad_inline unless ISMPC_ONE_LAUNCH=0 (form "two": tick + fallback launch);
    beyond N = 128, and with one instance per wavefront, ismpc_tick_affine + the fallback launch; the dense kernel has no fallback."""
    Rw = -(-N // 64)
    if lay == "dense":
        return ("dense", 64, Rw, 0, 1)
    if lay == "wave" or N > 128:
        return ("affine", 64, Rw, Rw, 2)
    R, RW = quad_rule(LANES[lay], N)
    return ("quad", LANES[lay], R, RW, 2) if form == "two" else ("quad_inline", LANES[lay], R, RW, 1)


def shape_of(info):
    return (info["family"], info["lanes"], info["R"], info["RW"], info["kernels"])


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


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@contextlib.contextmanager
def knobs(env):
    """The run-time knobs a handle reads at creation: saved, cleared, set, restored."""
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def new_handle(q, N, lay, **over):
    p = q.default_params(N=N)
    with knobs(dict(ENV[lay], **over)):
        return q.MPCSolver(q.reference_plan(params=p), params=p)


def handle(q, N, lay, **over):
    """The module's handles, keyed by (N, layout, overrides)."""
    return cached(("handle", N, lay, tuple(sorted(over.items()))), lambda: new_handle(q, N, lay, **over))


# ---- inputs: built and checked from the oracle alone ------------------------------------------------------------------------------------
def first_error_tick(O, outs):
    err = (outs["status"] & O.ST_ERROR_MASK) != 0
    return int(err.argmax()) if err.any() else len(outs)


def edge_inputs(O, N):
    """64 input records of horizon N, odd instances lifted."""
    odd = np.arange(B) % 2 == 1
    if N < 57:
        # states of the oracle's own closed loop at this horizon, before its first error tick, drawn with a fixed seed and perturbed
        outs, ins, _, _ = O.Oracle(O.default_params(N)).rollout(O.initial_state(), 0, 300)
        rng = np.random.default_rng(SEED_OF.get(N, SEED0 + N))
        tin = ins[rng.integers(0, first_error_tick(O, outs), B)].copy()
        tin["com_pos"][:, :2] += rng.uniform(-0.002, 0.002, (B, 2))
        tin["com_vel"][:, :2] += rng.uniform(-0.01, 0.01, (B, 2))
        dz = 0.12
    else:
        from quadruped_gait_generation_ismpc_amd import workload
        base = 200 if N > 150 else 100
        tin = workload.make_batch(base, 2 * B, scale=0.25, seed=SEED_OF.get(N, SEED0 + N))
        wide = workload.make_batch(base, 2 * B, scale=1.0, seed=SEED_OF.get(N, SEED0 + N))
        if N > 200:
            keep = tin["simulation_time"] < 1250                  # the footstep plan covers idx + 2 N
            tin, wide = tin[keep], wide[keep]
        tin, wide = tin[:B].copy(), wide[:B]
        # at a quarter of the generator's perturbation no horizontal QP beyond N = 100 ever changes its working set (the oracle alone, a dozen
        # seeds): every eighth instance keeps the same frame with the full perturbation, so that the knapsack loop has clipped samples to count
        tin[::8] = wide[::8]
        assert len(tin) == B
        dz = 0.25 if N >= 100 else 0.12
    tin["com_pos"][odd, 2] += dz
    tin["com_vel"][odd, 2] += 0.2
    return tin


def edge_case(O, N):
    """(inputs, oracle records, oracle info, oracle trajectories, active mask) of horizon N -- solved once, shared by every test and
    layout, never modified -- with the conditions the tests rely on asserted from the oracle alone."""
    def make():
        tin = edge_inputs(O, N)
        ref, info, traj = O.Oracle(O.default_params(N)).solve(tin, want_traj=True)
        good = (ref["status"] & O.ST_ERROR_MASK) == 0
        act = (ref["status"] & O.ST_Z_INEQ_ACTIVE) != 0
        grounded = (ref["status"] & O.ST_FLIGHT) == 0
        moved = (info["nwsr"][:, 1:] > 0).any(axis=1) & good
        print(f"edge_case[{N}]: error-free {int(good.sum())}, outside flight {int(grounded.sum())}, active {int(act.sum())}, "
              f"horizontal working-set changes on {int(moved.sum())} (max {int(info['nwsr'][:, 1:].max())})")
        assert good.sum() >= 56 and grounded.sum() >= 20, (N, good.sum(), grounded.sum())
        if 7 <= N <= 17 or N >= 57:
            assert act.sum() >= 24, (N, act.sum())
        if N >= 15:
            assert moved.any(), N
        assert ((ref["status"] & O.ST_Z_FAILED) == 0).all()
        for a in (tin, ref, info, traj):
            a.setflags(write=False)
        return tin, ref, info, traj, act
    return cached(("case", N), make)


def has_active(N):
    return 7 <= N <= 17 or N >= 57


def run_step(q, O, lay, N):
    """One 64-instance step of the module's handle of (layout, N): (records, launch_info right after the step)."""
    def make():
        tin = edge_case(O, N)[0]
        s = handle(q, N, lay)
        out = s.solve_batch(tin)
        return out, s.launch_info()
    return cached(("step", lay, N), make)


def check_against_oracle(q, N, lay, tin, out, ref, on_boundary=None):
    """The rules of test_gpu_parity.test_against_oracle_seeded, and the fallback's iteration byte on the active instances.
    on_boundary(record, band): the feasibility-band rule for a case that does not run with the default parameters and plan (which
    _on_feasibility_boundary builds); the rule and the band are the same."""
    ok = (ref["status"] & q.ST_ERROR_MASK) == 0
    assert ((out["status"] != ref["status"]) & ok).sum() == 0, (np.flatnonzero((out["status"] != ref["status"]) & ok), out["status"], ref["status"])
    diff = (out["status"] & q.ST_ERROR_MASK) != (ref["status"] & q.ST_ERROR_MASK)
    for b in np.where(diff)[0]:
        near = on_boundary(tin[b], 1e-9) if on_boundary is not None else _on_feasibility_boundary(q, N, tin[b], band=1e-9)
        assert near, (b, out["status"][b], ref["status"][b])
    assert_parity(q, out, ref, z_fallback=(lay != "dense"))
    act = (ref["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    both = act & (((ref["status"] | out["status"]) & q.ST_ERROR_MASK) == 0)
    if lay != "dense" and both.any():
        assert ((out["iters"][both] >> 16) & 255).min() >= 1


# ---- a. shape ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay,N", PAIRS)
def test_shape(q, O, lay, N):
    """launch_info() after the step equals the shape the rule gives: no id of this file silently runs a neighbouring shape."""
    _, info = run_step(q, O, lay, N)
    print(f"launch_info[{lay}-{N}] = {info}")
    assert shape_of(info) == expected_shape(lay, N), info
    assert info["batch"] == B and not info["sweep"] and not info["bound_order"]


def test_matrix_covers_both_sides_of_every_switch():
    """Every row of the shape table and every ceil(N / 64) appears on both sides of its switch (from the rule alone)."""
    for lanes, lay, switches in ((8, "lpi8", ((64, 8, 13), (104, 13, 16))), (16, "affine", ((64, 4, 7), (112, 7, 8)))):
        for n, lo, hi in switches:
            assert {n, n + 1} <= set(HORIZONS[lay]) and (quad_rule(lanes, n)[0], quad_rule(lanes, n + 1)[0]) == (lo, hi)
    assert (quad_rule(32, 64), quad_rule(32, 65)) == ((4, 1), (4, 2)) and {64, 65} <= set(HORIZONS["lpi32"])
    for lay in ("wave", "dense"):
        for n in (64, 128, 192):
            assert {n, n + 1} <= set(HORIZONS[lay]) and expected_shape(lay, n)[2] + 1 == expected_shape(lay, n + 1)[2]
    assert expected_shape("auto", 129)[0] == "affine" and expected_shape("lpi32", 128)[0] == "quad_inline"


# ---- b. oracle parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay,N", PAIRS)
def test_oracle_parity(q, O, lay, N):
    tin, ref, _, _, _ = edge_case(O, N)
    out, _ = run_step(q, O, lay, N)
    assert ((out["status"] & q.ST_Z_FAILED) == 0).all()
    check_against_oracle(q, N, lay, tin, out, ref)


# ---- c. decision trajectories with guards -----------------------------------------------------------------------------------------------
SENTINEL = -6.0221e+200          # a finite double no trajectory holds
SENTINEL_BYTE = 0xA5


@pytest.mark.parametrize("lay,N", PAIRS)
def test_decision_trajectories_with_guards(q, O, lay, N):
    """u_traj is 3 N doubles per instance with no slack: a padded lane that stores past its row lands in the next instance's row, or --
    for the last instance -- past the buffer.  The buffers are [64 + 2] instances with a guard row at each end; the call gets the address of
    row 1.  Bounds of test_decision_trajectories: 1e-6 of the largest |u_z|, 2e-6 absolute on x and y.  (dense flags the active instances
    only -- assert_parity(z_fallback=False) -- so their rows are not compared there.)"""
    import torch
    tin, ref, _, want, act = edge_case(O, N)
    plain, _ = run_step(q, O, lay, N)
    s = handle(q, N, lay)
    d_in = q.to_device(tin)
    traj = torch.empty((B + 2, 3, N), dtype=torch.float64, device="cuda:0")
    recs = torch.empty((B + 2, 80), dtype=torch.uint8, device="cuda:0")
    guard_t = np.full((3, N), SENTINEL).tobytes()
    guard_r = bytes([SENTINEL_BYTE]) * 80
    for b in (B, 1, 9):
        traj.fill_(SENTINEL); recs.fill_(SENTINEL_BYTE)
        u_view, o_view = traj[1:1 + b], recs[1:1 + b]
        assert u_view.data_ptr() == traj.data_ptr() + 3 * N * 8 and o_view.data_ptr() == recs.data_ptr() + 80
        s.solve_batch_torch(d_in[:b].contiguous(), o_view, u_traj=u_view)
        torch.cuda.synchronize()
        t, r = traj.cpu().numpy(), recs.cpu().numpy()
        assert t[0].tobytes() == guard_t and r[0].tobytes() == guard_r, (lay, N, b, "front guard")
        assert t[1 + b:].tobytes() == guard_t * (B + 1 - b) and r[1 + b:].tobytes() == guard_r * (B + 1 - b), (lay, N, b, "rows past the batch")
        t, out = t[1:1 + b], np.ascontiguousarray(r[1:1 + b]).view(q.TICK_OUT).reshape(-1)
        assert not (t == SENTINEL).any(), (lay, N, b, np.argwhere(t == SENTINEL)[:4])
        assert out.tobytes() == plain[:b].tobytes()
        assert np.array_equal(t[:, :, 0], out["u0"])
        ok = ((ref["status"][:b] | out["status"]) & q.ST_ERROR_MASK) == 0
        if lay == "dense":
            ok &= ~act[:b]
        if b == B:
            assert ok.sum() >= 24
        if ok.any():
            w = want[:b]
            ez = np.abs(t[ok, 0] - w[ok, 0]).max() / np.abs(w[ok, 0]).max()
            exy = np.abs(t[ok, 1:] - w[ok, 1:]).max()
            print(f"u_traj[{lay}-{N}-b{b}]: |du_z| / max|u_z| = {ez:.3e}, |du_xy| = {exy:.3e}")
            assert ez <= 1e-6 and exy <= 2e-6, (lay, N, b, ez, exy)


# ---- d. batch independence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay,N", PAIRS)
def test_batch_independence(q, O, lay, N):
    tin = edge_case(O, N)[0]
    full, _ = run_step(q, O, lay, N)
    s = handle(q, N, lay)
    for b in (1, 9, 63):
        assert s.solve_batch(tin[:b]).tobytes() == full[:b].tobytes(), (lay, N, b)
    perm = np.random.default_rng(64).permutation(B)
    assert s.solve_batch(tin[perm]).tobytes() == full[perm].tobytes()


# ---- e. vertical fallback forms ---------------------------------------------------------------------------------------------------------
FORM_PAIRS = [(lay, N) for lay in ("affine", "lpi8", "lpi32") for N in HORIZONS[lay] if has_active(N)]


@pytest.mark.parametrize("lay,N", FORM_PAIRS)
def test_fallback_forms_agree_bytewise(q, O, lay, N):
    """ISMPC_ONE_LAUNCH=3 (64 instances are resident: ismpc_tick_quad_inline runs the fallback body itself) and =0 (ismpc_tick_quad, the
    deferred list, ismpc_tick_affine_fallback at RW = ceil(N / 64)): the same bytes, nothing unsolved, the oracle's active set."""
    tin, ref, _, _, act = edge_case(O, N)
    outs = {}
    for form, v in (("one", "3"), ("two", "0")):
        s = new_handle(q, N, lay, ISMPC_ONE_LAUNCH=v)
        try:
            outs[form] = s.solve_batch(tin)
            info = s.launch_info()
            assert s.fallback_counters() == (0, 0, 0, 0)
        finally:
            s.close()
        print(f"launch_info[{lay}-{N}-{form}] = {info}")
        assert shape_of(info) == expected_shape(lay, N, form), info
    assert outs["one"].tobytes() == outs["two"].tobytes()
    assert outs["one"].tobytes() == run_step(q, O, lay, N)[0].tobytes()
    assert ((outs["one"]["status"] & q.ST_Z_FAILED) == 0).all()
    assert np.array_equal((outs["one"]["status"] & q.ST_Z_INEQ_ACTIVE) != 0, act)


@pytest.mark.parametrize("lay,N", [(lay, N) for lay in ("affine", "lpi8", "lpi32", "wave") for N in (9, 65, 128)])
def test_fallback_working_set_in_the_pool_changes_no_byte(q, O, lay, N):
    """ISMPC_Z_LDS_Q=2: the fallback's working set leaves the LDS window for its pool slot after two entries."""
    tin, _, info, _, act = edge_case(O, N)
    print(f"oracle: vertical working-set changes on the active instances, max {int(info['nwsr'][act, 0].max())}")
    assert (info["nwsr"][act, 0] >= 3).any()                   # (the oracle alone) some working set does outgrow two entries
    s = new_handle(q, N, lay, ISMPC_Z_LDS_Q=2)
    try:
        out = s.solve_batch(tin)
    finally:
        s.close()
    assert out.tobytes() == run_step(q, O, lay, N)[0].tobytes()


# ---- f. closed loops --------------------------------------------------------------------------------------------------------------------
LOOPS = [("affine", N) for N in (8, 9, 64, 65, 128)] + [("lpi8", 104), ("lpi8", 105), ("affine", 112), ("affine", 113)]


@pytest.mark.parametrize("lay,N", LOOPS)
def test_closed_loops(q, O, lay, N):
    """ismpc_rollout_quad at the edge shapes: byte for byte the per-tick loop (ISMPC_ROLLOUT=host) and the disturbed rollout without
    pushes, within TOL of the oracle's closed loop with equal statuses, up to the oracle's first error tick (short horizons lose
    feasibility late in the gait in the oracle itself)."""
    import torch
    st0 = O.initial_state().view(q.TICK_IN)
    ref, _, _, fin = O.Oracle(O.default_params(N)).rollout(st0, 0, 120)
    ticks = min(120, first_error_tick(O, ref))
    assert ticks >= 40, (N, ticks)
    recs = np.repeat(st0, 2)
    a, h = handle(q, N, lay), handle(q, N, lay, ISMPC_ROLLOUT="host")
    sa, sh, sm = q.to_device(recs), q.to_device(recs), q.to_device(recs)
    ta = a.rollout_torch(sa, 0, ticks)
    torch.cuda.synchronize()
    info = a.launch_info()
    th = h.rollout_torch(sh, 0, ticks)
    tm, _ = a.rollout_mc_torch(sm, 0, ticks, stride=1)
    torch.cuda.synchronize()
    info_mc = a.launch_info()
    print(f"launch_info[rollout-{lay}-{N}] = {info}; ticks {ticks}")
    R, RW = quad_rule(LANES[lay], N)
    assert shape_of(info) == ("rollout_quad", LANES[lay], R, RW, 2), info
    assert info_mc["mc"] is True and shape_of(info_mc) == shape_of(info), info_mc
    assert torch.equal(ta, th) and torch.equal(sa, sh)
    assert torch.equal(tm, ta) and torch.equal(sm, sa)
    out = q.from_device(ta, q.TICK_OUT)
    for i in range(2):
        assert np.array_equal(out["status"][:, i], ref["status"][:ticks]), (out["status"][:, i], ref["status"][:ticks])
        assert rel_com(out[:, i], ref[:ticks]).max() <= TOL
        assert np.abs(out["com_vel"][:, i] - ref["com_vel"][:ticks]).max() <= TOL
    if ticks == 120:
        end = q.from_device(sa, q.TICK_IN)
        for k in ("mpc_iter", "control_iter", "footstep_counter", "simulation_time"):
            assert end[k][0] == fin[k][0], k


# ---- g. sweeps --------------------------------------------------------------------------------------------------------------------------
SWEEP_N = [1, 8, 65, 129, 256]


def sweep_handle(q, N):
    from quadruped_gait_generation_ismpc_amd import workload

    def make():
        sets = workload.make_sweep_params(3, N=N)
        return sets, q.MPCSolver.sweep(q.reference_plan(params=sets[0]), sets)
    return cached(("sweep", N), make)


@pytest.mark.parametrize("N", SWEEP_N)
def test_sweep_edge_tables(q, N):
    """The sweep's device-built tables (Newton-Schulz GEMM in tiles of 64 / 128 / 256: 65 and 129 are the first horizons inside the 128 and
    256 tiles, 1 and 8 nearly empty ones, 256 a full one) against the host's long-double build, within the bound of
    test_gpu_sweep.test_sweep_other_horizons: 1e-11 of each table's largest entry.

    N = 256 missed that bound when this test was written (S W_p 1.7e-10, Hinv S' 1.3e-11 and the affine tables 1.06e-11 on set 2), and not
    through padding: the fp64 Newton-Schulz iterate carries cond(H) eps of unstructured noise, which the running sums of S amplify.  The
    build now ends with one Newton step from a double-double residual (sweep_residual_dd) and builds the right-hand sides in
    double-double; what is left is the rounding of H's own fp64 entries: at N = 256 every kind <= 3.2e-12 (Hinv S' of set 2), at
    N = 129 <= 4.9e-13, at N = 65 <= 6.1e-14, at N = 8 <= 6.7e-16."""
    sets, s = sweep_handle(q, N)
    errs = [s.sweep_verify_tables(k) for k in range(3)]
    for k, err in enumerate(errs):
        print(f"sweep_verify_tables[{N}, set {k}] = {err}")
    for k, err in enumerate(errs):
        assert max(err.values()) <= 1e-11, (k, err)


@pytest.mark.parametrize("N", SWEEP_N)
def test_sweep_edge_batch(q, O, N):
    """63 instances over three sets against one oracle per set, by the rules of test_gpu_sweep.test_sweep_other_horizons."""
    sets, s = sweep_handle(q, N)
    tin = edge_case(O, N)[0][:63].copy()
    tin["reserved"] = np.arange(63) % 3
    refs = []
    for k in range(3):
        m = np.flatnonzero(tin["reserved"] == k)
        op = O.default_params(N, mass=sets[k].mass, h_des=sets[k].h_des, q_p=sets[k].q_p, q_u=sets[k].q_u, q_v=sets[k].q_v, foot_width=sets[k].foot_width)
        refs.append((m, O.Oracle(op).solve(tin[m])[0]))
    n_good = [int(((r["status"] & O.ST_ERROR_MASK) == 0).sum()) for _, r in refs]
    print(f"sweep[{N}]: oracle error-free per set {n_good} of 21")
    assert min(n_good) >= 8, n_good
    out = s.solve_batch(tin)
    info = s.launch_info()
    print(f"launch_info[sweep-{N}] = {info}")
    assert info["sweep"] and ((info["family"], info["lanes"]) == ("affine", 64) if N > 128 else (info["lanes"], info["R"], info["RW"]) == (16,) + quad_rule(16, N))
    assert ((out["status"] & (q.ST_BAD_INDEX | q.ST_Z_FAILED)) == 0).all()
    for m, ref in refs:
        ok = ((ref["status"] | out["status"][m]) & q.ST_ERROR_MASK) == 0
        assert ok.sum() >= 8
        assert rel_com(out[m], ref)[ok].max() <= TOL and (out["status"][m][ok] == ref["status"][ok]).all(), (N, rel_com(out[m], ref)[ok].max())
