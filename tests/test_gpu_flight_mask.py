"""The lane-group tick core keeps a lane group in the knapsack Newton loop only while something of its stage 3 is stored: a group in
flight (lambda_0 <= gate, MPCSolver.cpp:322), a gated group (skipped tick, bad index) and a tail group that recomputes the last instance
are never live (per-tick kernels; the closed loop keeps its unmasked loop and is pinned here to stay byte-equal).  That is a change of
SCHEDULE: which groups keep a wavefront iterating.  No record may depend on it, so every test here compares bytes -- an instance's
record against the record the same instance gets with other wave-mates, in another slot, in another launch form -- and the mixed batch
once against the CPU oracle at the project's TOL.

Instances come from workload.make_batch(100, 4096), picked by the device's own first solve at the layout under test:
  F  flight instances (ST_FLIGHT);
  H  stage-3 instances whose slower axis took at least 4 Newton passes (the ones a flight wave-mate used to iterate beside);
  E  stage-3 instances with one pass on both axes (the ones that wait).
"""
import numpy as np
import pytest

from test_gpu_parity import TOL, assert_parity                                                # noqa: F401  (TOL: assert_parity's bound)
from test_gpu_dispatch_parity import BATCH, expected_step, fresh_solver, knobs, lift, matrix_batch

pytestmark = pytest.mark.gpu

N = 100
LANES = (8, 16, 32)


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


def iters_xy(out):
    return out["iters"] & 255, (out["iters"] >> 8) & 255


_cache = {}


def mixed_case(q, lanes):
    """Per layout, solved once and shared: the handle, the pool, the three groups of instances, batch M and its records."""
    if lanes in _cache:
        return _cache[lanes]
    from quadruped_gait_generation_ismpc_amd import workload
    s = fresh_solver(q, N, lpi=lanes)
    pool = workload.make_batch(N, 4096)
    first = s.solve_batch(pool)
    assert s.launch_info()["lanes"] == lanes
    itx, ity = iters_xy(first)
    clean = first["status"] == 0                                                           # stage 3 ran, nothing deferred, nothing flagged
    F = np.flatnonzero(first["status"] == q.ST_FLIGHT)
    H = np.flatnonzero(clean & (np.maximum(itx, ity) >= 4))
    E = np.flatnonzero(clean & (itx == 1) & (ity == 1))
    print(f"lanes {lanes}: flight {len(F)}, stage 3 with >= 4 passes {len(H)}, stage 3 with 1 + 1 passes {len(E)} of 4096")
    assert len(F) >= 8 and len(H) >= 8 and len(E) >= 8, (len(F), len(H), len(E))
    ipw = 64 // lanes
    B = 3 * ipw + max(1, ipw // 2)                                                         # three wavefronts and a partial one
    assert B % ipw != 0
    # slot i holds kind i mod 3 (F, H, E): every wavefront of 4 or 8 instances holds all three, the two-instance wavefronts of the
    # 32-lane layout every pair of them
    kind = np.arange(B) % 3
    src = np.empty(B, dtype=np.int64)
    for k, grp in enumerate((F, H, E)):
        slots = np.flatnonzero(kind == k)
        src[slots] = grp[np.arange(len(slots)) % len(grp)]
    M = pool[src].copy()
    gated = 2                                                                              # an E slot (first wavefront; second at 32 lanes) becomes a bad index
    M["simulation_time"][gated] = 1700.0                                                   # (the midpoint window guard, as test_passthrough_rules)
    kind[gated] = 3
    # the E instances that replace the F ones in batch S: other ones than M already holds where the pool has them
    spare = E[::-1]
    case = dict(s=s, pool=pool, first=first, src=src, F=F, H=H, E=E, B=B, kind=kind, M=M, gated=gated, spare=spare, out=s.solve_batch(M))
    _cache[lanes] = case
    return case


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for key, case in _cache.items():
        if key != "matrix":
            case["s"].close()
    _cache.clear()


@pytest.mark.parametrize("lanes", LANES)
def test_mixed_wavefronts_keep_their_properties(q, O, lanes):
    """Batch M against the oracle, and what the mask must not touch: the heavy instances keep their pass counts, the flight instances
    report no pass at all, the gated one is passed through."""
    c = mixed_case(q, lanes)
    M, out, kind = c["M"], c["out"], c["kind"]
    assert c["s"].launch_info()["lanes"] == lanes and c["s"].launch_info()["batch"] == c["B"]
    ref, _ = O.Oracle(O.default_params(N)).solve(M)
    ok = ((ref["status"] | out["status"]) & q.ST_ERROR_MASK) == 0
    assert ok.sum() == c["B"] - 1                                                          # everything but the gated instance is compared
    assert_parity(q, out, ref, ok)
    assert out["status"][c["gated"]] == q.ST_BAD_INDEX == ref["status"][c["gated"]]
    assert np.array_equal(out["com_pos"][c["gated"]], M["com_pos"][c["gated"]]) and np.all(out["u0"][c["gated"]] == 0) and out["iters"][c["gated"]] == 0
    itx, ity = iters_xy(out)
    f, h, e = kind == 0, kind == 1, kind == 2
    assert (np.maximum(itx, ity)[h] >= 4).all() and (out["status"][h] == 0).all()
    assert (itx[e] == 1).all() and (ity[e] == 1).all() and (out["status"][e] == 0).all()
    assert (out["iters"][f] == 0).all() and (out["status"][f] == q.ST_FLIGHT).all()
    assert np.all(out["u0"][f] == 0.0)
    # every instance has the record of the first solve, where it sat among other wave-mates
    keep = kind != 3
    assert out[keep].tobytes() == c["first"][c["src"][keep]].tobytes()


@pytest.mark.parametrize("lanes", LANES)
def test_records_do_not_depend_on_flight_wave_mates(q, lanes):
    """Batch S = M with every flight instance replaced by a one-pass stage-3 instance: whoever was not replaced has the same bytes.
    And the flight instances alone, in wavefronts of their own, have the bytes they have in M."""
    c = mixed_case(q, lanes)
    s, M, out, kind = c["s"], c["M"], c["out"], c["kind"]
    f = kind == 0
    S = M.copy()
    S[f] = c["pool"][c["spare"][np.arange(f.sum()) % len(c["spare"])]]
    out_s = s.solve_batch(S)
    assert ((out_s["status"][f] & q.ST_FLIGHT) == 0).all()                                  # the replacements do run stage 3
    assert out_s[~f].tobytes() == out[~f].tobytes()
    alone = s.solve_batch(M[f])
    assert alone.tobytes() == out[f].tobytes()


@pytest.mark.parametrize("lanes", LANES)
def test_decision_trajectories_of_the_mixed_batch(q, lanes):
    """The u_traj call: the same records, and the x and y rows of a flight instance are all 0."""
    import torch
    c = mixed_case(q, lanes)
    s, M, out, kind = c["s"], c["M"], c["out"], c["kind"]
    traj = torch.full((c["B"], 3, N), np.nan, dtype=torch.float64, device="cuda:0")
    d_out = s.solve_batch_torch(q.to_device(M), u_traj=traj)
    torch.cuda.synchronize()
    got = q.from_device(d_out, q.TICK_OUT)
    assert got.tobytes() == out.tobytes()
    f, h = kind == 0, kind == 1
    itx, ity = iters_xy(got)
    assert (got["iters"][f] == 0).all() and (got["status"][f] == q.ST_FLIGHT).all()
    assert (np.maximum(itx, ity)[h] >= 4).all()
    t = traj.cpu().numpy()
    assert not np.isnan(t).any()
    assert np.all(t[f, 1:] == 0.0) and np.array_equal(t[f, 0, 0], got["u0"][f, 0])
    assert np.all(t[c["gated"]] == 0.0)
    assert np.array_equal(t[:, :, 0], got["u0"])
    assert (np.abs(t[h, 1:]).max(axis=(1, 2)) > 0.0).all()


# ---- permutation invariance at a non-resident size --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "two"])
def test_permutation_invariance_beyond_the_resident_size(q, cus, form):
    """20 001 instances (a quarter of them deferred, the rest spread over the whole gait: flight and stance side by side in every
    wavefront) in the order given and in a fixed random order: every instance has the same bytes wherever it sits."""
    if "matrix" not in _cache:
        _cache["matrix"] = matrix_batch(N)
    tin = _cache["matrix"]
    perm = np.random.default_rng(20001).permutation(BATCH)
    s = fresh_solver(q, N, form=form if form == "two" else None)
    try:
        a = s.solve_batch(tin)
        info = s.launch_info()
        b = s.solve_batch(tin[perm])
    finally:
        s.close()
    print(f"launch_info[{form}] = {info}")
    assert info == expected_step(cus, BATCH, N, one_launch=0 if form == "two" else None)
    if form == "one":
        assert (info["family"], info["lanes"], info["R"], info["kernels"]) == ("quad_one", 8, 13, 1)
    else:
        assert (info["family"], info["lanes"], info["R"], info["kernels"]) == ("quad", 8, 13, 2)
    fl = (a["status"] & q.ST_FLIGHT) != 0
    print(f"flight {fl.mean():.3f}, deferred {((a['status'] & q.ST_Z_INEQ_ACTIVE) != 0).mean():.3f}")
    assert 0.05 < fl.mean() < 0.6 and ((a["status"] & q.ST_Z_INEQ_ACTIVE) != 0).mean() > 0.2
    assert (a["iters"][fl & ((a["status"] & q.ST_Z_INEQ_ACTIVE) == 0)] == 0).all()
    assert b.tobytes() == a[perm].tobytes()


# ---- closed loop: phases change inside a launch, instances are parked beside running ones -----------------------------------------------------------
ROLL_LANES, ROLL_TICKS, ROLL_FRAME = 16, 12, 399
ROLL_B = 3 * (64 // ROLL_LANES) + 2


def rollout_states(parking):
    """Perturbed copies of the nominal closed loop's state at frame ROLL_FRAME, in the flight phase of the gait, a few ticks before touch
    down.  parking: the second instance of every wavefront starts far above h_des with an upward velocity (lift of the dispatch test): its
    vertical inequality rows are active at the first tick, the first launch parks it and the resume launch finishes it."""
    from quadruped_gait_generation_ismpc_amd import workload
    table, lo, hi = workload.load_preroll(N)
    st = np.repeat(table[ROLL_FRAME:ROLL_FRAME + 1], ROLL_B)
    assert st["simulation_time"][0] == ROLL_FRAME
    u = np.random.Generator(np.random.Philox(key=4600)).uniform(-1.0, 1.0, (ROLL_B, 6))
    P = workload.PERTURB
    st["com_pos"][:, :2] += P["pos_xy"] * u[:, 0:2]; st["com_vel"][:, :2] += P["vel_xy"] * u[:, 2:4]
    st["com_pos"][:, 2] += P["pos_z"] * u[:, 4]; st["com_vel"][:, 2] += P["vel_z"] * u[:, 5]
    sel = np.arange(ROLL_B) % 4 == 1
    if parking:
        assert np.array_equal(lift(st, N), sel)
    return st, sel


def test_rollout_is_unchanged_across_phases_and_beside_parked_instances(q):
    import torch
    frame = ROLL_FRAME + 1
    st_p, sel = rollout_states(True)
    st_n, _ = rollout_states(False)
    assert st_p[~sel].tobytes() == st_n[~sel].tobytes()
    with knobs(ISMPC_PATH="affine", ISMPC_LPI=ROLL_LANES):
        p = q.default_params(N=N)
        roll = q.MPCSolver(q.reference_plan(params=p), params=p)
    with knobs(ISMPC_PATH="affine", ISMPC_LPI=ROLL_LANES, ISMPC_ROLLOUT="host"):
        host = q.MPCSolver(q.reference_plan(params=p), params=p)
    try:
        dp, dn, dh = q.to_device(st_p), q.to_device(st_n), q.to_device(st_p)
        tp = roll.rollout_torch(dp, frame, ROLL_TICKS)
        info = roll.launch_info()
        tn = roll.rollout_torch(dn, frame, ROLL_TICKS)
        th = host.rollout_torch(dh, frame, ROLL_TICKS)
        torch.cuda.synchronize()
        info_h = host.launch_info()
    finally:
        roll.close(); host.close()
    print(f"launch_info[rollout] = {info}; [host loop] = {info_h}")
    assert (info["family"], info["lanes"], info["R"], info["kernels"], info["batch"]) == ("rollout_quad", ROLL_LANES, 7, 2, ROLL_B)
    assert info_h["family"] != "rollout_quad" and info_h["lanes"] == ROLL_LANES
    op, on = q.from_device(tp, q.TICK_OUT), q.from_device(tn, q.TICK_OUT)                  # [ticks, B]
    fl = (on["status"] & q.ST_FLIGHT) != 0
    print("flight per tick (nominal batch):", fl.sum(1).tolist())
    # in flight at the first tick and in stance at a later tick of the same launch: the mask cannot be taken once per launch
    changes = fl[0] & ~fl[-1] & ((on["status"][-1] & (q.ST_ERROR_MASK | q.ST_Z_INEQ_ACTIVE)) == 0)
    assert changes.sum() >= ROLL_B // 2, changes
    itx, ity = iters_xy(on)
    assert (on["iters"][fl] == 0).all() and (itx[-1][changes] >= 1).all() and (ity[-1][changes] >= 1).all()
    # the parking instances were parked at the first tick and finished by the resume launch
    assert ((op["status"][0, sel] & q.ST_Z_INEQ_ACTIVE) != 0).all() and ((on["status"] & q.ST_Z_INEQ_ACTIVE) == 0).all()
    assert ((op["status"] & q.ST_Z_FAILED) == 0).all()
    # the others do not notice what their wave-mate is
    assert op[:, ~sel].tobytes() == on[:, ~sel].tobytes()
    assert torch.equal(dp.cpu()[~sel], dn.cpu()[~sel])
    # ... and the launch is the per-tick loop, byte for byte: trajectories and final states
    assert torch.equal(tp, th) and torch.equal(dp, dh)
