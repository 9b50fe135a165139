"""The knapsack Newton loop of the per-tick lane-group kernels keeps its live flags in two wave-wide lane masks (tick_group_core in
csrc/ismpc_b_group.hpp): a group leaves an axis when its mask bit goes, the wavefront leaves the loop when both masks are empty.  That
is bookkeeping only: every QP must see the iterate sequence it saw with per-lane flags, whatever its wave-mates do.  So every test here
compares BYTES -- an instance's record in a batch against the record the same handle returns for that instance launched alone, in a batch
of eight copies of itself (one full wavefront at 8 lanes per instance, whose groups all finish together) -- and the mixed batch once per
form against the CPU oracle within the tolerances of tests/test_gpu_parity.py (TOL, assert_parity).

Inputs, chosen on the CPU (scripts/knapsack_model.py's replay of the kernel's Newton rule on the oracle's vertical trajectory gives the
sum passes per axis; the oracle gives the status):

  MIX = make_batch(100, 24, scale=1.0, seed=5303): the oracle flags nothing (status 0 on 21, ST_FLIGHT on 3: instances 2, 8, 18).  Sum
    passes (x, y) of the 21 stage-3 instances: (0, 0) on 13, (2, 0) on 5 and 11, (4, 0) on 19, (0, 1) on 20 and 22, (0, 3) on 12, (0, 4) on
    21.  At 8 lanes per instance the third wavefront (16 .. 23) holds a flight group, groups that never update, one that leaves x after
    four updates while y is long done, and one that does the same on y; the second one holds (2, 0) beside (0, 3).
  HARD = make_batch(100, 24, scale=4.0, seed=5300): both axes update in most instances ((3, 4), (2, 5), (4, 4), (3, 2) ...), 7 are in
    flight, 15 end with everything saturated on an axis (oracle: ST_X_INFEASIBLE on 8, ST_Y_INFEASIBLE on 3, both on 4), instances 15 and
    16 are feasible.  Its infeasible instances are compared with the oracle by status only (there is no solution to compare).

The kernel reports 1 + (sum passes) per axis in `iters`; the mixed test asserts the counts above on the device's records, so the batch
keeps holding the cases it was picked for.
"""
import numpy as np
import pytest

from test_gpu_parity import TOL, assert_parity                                                # noqa: F401  (TOL: assert_parity's bound)
from test_gpu_dispatch_parity import knobs

pytestmark = pytest.mark.gpu

N = 100
FORMS = ("resident", "two", "one")
FAMILY = {"resident": "quad_inline", "two": "quad", "one": "quad_one"}
SHAPE_R = {8: 13, 16: 7, 32: 4}
MIX_PASSES = {5: (2, 0), 11: (2, 0), 19: (4, 0), 20: (0, 1), 22: (0, 1), 12: (0, 3), 21: (0, 4)}        # every other stage-3 instance: (0, 0)
MIX_FLIGHT = (2, 8, 18)
HARD_FEASIBLE = (15, 16)
HARD_FLIGHT = (0, 2, 4, 7, 14, 18, 21)


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


def iters_xy(out):
    return out["iters"] & 255, (out["iters"] >> 8) & 255


def make_solver(q, form, lanes, p=None, plan=None):
    """As tests/test_gpu_workgroup_width.py forces a form: `one` is a multi-plan handle with one set and one plan (never resident, so it
    takes ismpc_tick_quad_one at every batch size); the layout by ISMPC_LPI."""
    p = p if p is not None else q.default_params(N=N)
    plan = plan if plan is not None else q.reference_plan(params=p)
    with knobs(ISMPC_LPI=lanes, ISMPC_ONE_LAUNCH={"resident": None, "two": 0, "one": 3}[form]):
        return q.MPCSolver.plans([plan], p) if form == "one" else q.MPCSolver(plan, params=p)


def check_form(s, form, lanes, batch):
    info = s.launch_info()
    assert (info["family"], info["lanes"], info["R"], info["batch"]) == (FAMILY[form], lanes, SHAPE_R[lanes], batch), info


def alone(s, tin):
    """Each instance in a batch of eight copies of itself; the eight records agree, the first one is returned."""
    rows = []
    for i in range(len(tin)):
        o = s.solve_batch(np.repeat(tin[i:i + 1], 8))
        assert all(o[k].tobytes() == o[0].tobytes() for k in range(8)), i
        rows.append(o[:1])
    return np.concatenate(rows)


@pytest.fixture(scope="module")
def batches(O):
    """MIX, HARD and the oracle's records of both: computed once, never modified."""
    from quadruped_gait_generation_ismpc_amd import workload
    mix = workload.make_batch(N, 24, scale=1.0, seed=5303)
    hard = workload.make_batch(N, 24, scale=4.0, seed=5300)
    orc = O.Oracle(O.default_params(N))
    ref_mix, ref_hard = orc.solve(mix)[0], orc.solve(hard)[0]
    assert (ref_mix["status"][list(MIX_FLIGHT)] == O.ST_FLIGHT).all() and (np.delete(ref_mix["status"], MIX_FLIGHT) == 0).all()
    assert (ref_hard["status"][list(HARD_FEASIBLE)] == 0).all() and (ref_hard["status"][list(HARD_FLIGHT)] == O.ST_FLIGHT).all()
    inf = np.delete(ref_hard["status"], HARD_FEASIBLE + HARD_FLIGHT)
    assert len(inf) == 15 and ((inf & (O.ST_X_INFEASIBLE | O.ST_Y_INFEASIBLE)) != 0).all() and ((inf & ~3) == 0).all()
    for a in (mix, hard, ref_mix, ref_hard):
        a.setflags(write=False)
    return mix, hard, ref_mix, ref_hard


@pytest.fixture(scope="module")
def forms(q, batches):
    """Per (form, layout): the handle and the record of every MIX and HARD instance launched alone."""
    mix, hard = batches[0], batches[1]
    made = {}
    try:
        for lanes in (8, 16, 32):
            for form in FORMS:
                s = make_solver(q, form, lanes)
                made[(form, lanes)] = [s, None, None]
                a_mix, a_hard = alone(s, mix), alone(s, hard)
                check_form(s, form, lanes, 8)
                a_mix.setflags(write=False); a_hard.setflags(write=False)
                made[(form, lanes)][1:] = [a_mix, a_hard]
        yield made
    finally:
        for s, _, _ in made.values():
            s.close()


# ---- mixed finishing order in one wavefront, every layout, every launch form -------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [8, 16, 32])
@pytest.mark.parametrize("form", FORMS)
def test_mixed_finishing_order(q, batches, forms, form, lanes):
    mix, hard, ref_mix, ref_hard = batches
    s, a_mix, a_hard = forms[(form, lanes)]
    out = s.solve_batch(mix)
    check_form(s, form, lanes, 24)
    itx, ity = iters_xy(out)
    print(f"[{form}-{lanes}] MIX status {out['status'].tolist()} passes {list(zip((itx - 1).tolist(), (ity - 1).tolist()))}")
    assert out.tobytes() == a_mix.tobytes(), np.flatnonzero([out[i].tobytes() != a_mix[i].tobytes() for i in range(24)])
    assert_parity(q, out, ref_mix, np.ones(24, bool))
    for i in range(24):
        want = (0, 0) if i in MIX_FLIGHT else tuple(1 + v for v in MIX_PASSES.get(i, (0, 0)))
        assert (itx[i], ity[i]) == want, (i, itx[i], ity[i], want)
    outh = s.solve_batch(hard)
    itx, ity = iters_xy(outh)
    print(f"[{form}-{lanes}] HARD status {outh['status'].tolist()} passes {list(zip((itx - 1).tolist(), (ity - 1).tolist()))}")
    assert outh.tobytes() == a_hard.tobytes(), np.flatnonzero([outh[i].tobytes() != a_hard[i].tobytes() for i in range(24)])
    assert np.array_equal(outh["status"], ref_hard["status"])
    ok = np.zeros(24, bool); ok[list(HARD_FEASIBLE + HARD_FLIGHT)] = True
    assert_parity(q, outh, ref_hard, ok)
    both = (itx >= 3) & (ity >= 3) & (itx != ity)
    assert both.sum() >= 4, both                                                             # both axes update, and finish in different passes
    # the two batches interleaved (a healthy group beside an all-saturated one in every wavefront): still the records of each alone
    inter = np.empty(48, dtype=mix.dtype); inter[0::2] = mix; inter[1::2] = hard
    outi = s.solve_batch(inter)
    assert outi[0::2].tobytes() == a_mix.tobytes() and outi[1::2].tobytes() == a_hard.tobytes()


def test_forms_and_layout_agree(forms):
    """Per layout the three forms return the same bytes (the multi-plan instantiation and the two-launch form share the core)."""
    for lanes in (8, 16, 32):
        for form in ("two", "one"):
            assert forms[(form, lanes)][1].tobytes() == forms[("resident", lanes)][1].tobytes(), (form, lanes)
            assert forms[(form, lanes)][2].tobytes() == forms[("resident", lanes)][2].tobytes(), (form, lanes)


# ---- wave-mates that are never live ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool65():
    from quadruped_gait_generation_ismpc_amd import workload
    t = workload.make_batch(N, 65, scale=1.0, seed=5303)            # its first 24 are MIX
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def alone65(q, forms, pool65):
    return {form: np.concatenate([forms[(form, 8)][1], alone(forms[(form, 8)][0], pool65[24:])]) for form in FORMS}


@pytest.mark.parametrize("batch", [1, 7, 9, 63, 65])
@pytest.mark.parametrize("form", FORMS)
def test_tail_groups_are_never_live(q, forms, pool65, alone65, form, batch):
    """Tail groups recompute the last instance and store nothing; a last wavefront with one valid group (9, 65)."""
    s = forms[(form, 8)][0]
    out = s.solve_batch(pool65[:batch])
    check_form(s, form, 8, batch)
    assert out.tobytes() == alone65[form][:batch].tobytes(), np.flatnonzero([out[i].tobytes() != alone65[form][i].tobytes() for i in range(batch)])


@pytest.mark.parametrize("form", FORMS)
def test_flight_beside_a_group_that_updates(q, batches, forms, form):
    """Instance 18 of MIX is in flight, 19 needs four updates on x, 21 four on y: in flight first, in flight second."""
    mix = batches[0]
    s, a_mix, _ = forms[(form, 8)]
    for pair in ([18, 19], [19, 18], [18, 21], [21, 18]):
        out = s.solve_batch(mix[pair])
        check_form(s, form, 8, 2)
        assert out.tobytes() == a_mix[pair].tobytes(), pair
        fl = out["status"] == q.ST_FLIGHT
        assert fl.tolist() == [i == 18 for i in pair] and (out["iters"][fl] == 0).all() and (np.maximum(*iters_xy(out))[~fl] == 5).all()


@pytest.mark.parametrize("form", FORMS)
def test_gated_instance_beside_running_ones(q, O, batches, form):
    """mpc_dt = 2 control_dt (tick divisor 2): the instance with an odd control_iter is skipped and never live; its wave-mates keep the
    bytes they have alone, and so does it."""
    p = q.default_params(N=N, mpc_dt=0.02)
    s = make_solver(q, form, 8, p=p, plan=O.reference_plan(mpc_dt=0.02))
    try:
        t = batches[0][16:24].copy()
        t["control_iter"] = 2 * (t["control_iter"] // 2)
        t["control_iter"][3] += 1                                     # MIX 19, the one with four updates on x
        one = alone(s, t)
        out = s.solve_batch(t)
        check_form(s, form, 8, 8)
    finally:
        s.close()
    assert out.tobytes() == one.tobytes()
    assert out["status"][3] == q.ST_TICK_SKIPPED and out["iters"][3] == 0 and np.array_equal(out["com_pos"][3], t["com_pos"][3])
    run = np.arange(8) != 3
    assert ((out["status"][run] & (q.ST_TICK_SKIPPED | q.ST_BAD_INDEX)) == 0).all()
    # the others did run stage 3 but for the one in flight.  (These states belong to the 10 ms gait: at 20 ms the oracle finds x or both axes
    # infeasible on all of them -- groups that stay live until everything is saturated, beside the gated one.)
    ref = O.Oracle(O.default_params(N, mpc_dt=0.02), O.reference_plan(mpc_dt=0.02)).solve(t)[0]
    X, XY = O.ST_X_INFEASIBLE, O.ST_X_INFEASIBLE | O.ST_Y_INFEASIBLE
    assert ref["status"].tolist() == [X, XY, O.ST_FLIGHT, O.ST_TICK_SKIPPED, XY, X, X, XY]
    assert np.array_equal(out["status"], ref["status"]) and (np.maximum(*iters_xy(out))[run] >= 2).sum() == 6


# ---- degenerate QPs --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_whole_horizon_in_flight(q, O, batches, form):
    """lambda_gate above every lambda_j: every sample of the horizon is in flight, a_n = 0 everywhere, q0 = 0.  (q0 = 0 implies that sample 0
    is in flight too, so such a group is never live; tau is set before the loop and nothing of stage 3 is stored.)  Against the oracle."""
    p = q.default_params(N=N, lambda_gate=1.0e9)
    s = make_solver(q, form, 8, p=p)
    try:
        t = batches[0][:9]
        out = s.solve_batch(t)
        check_form(s, form, 8, 9)
        one = alone(s, t)
    finally:
        s.close()
    ref = O.Oracle(O.default_params(N, lambda_gate=1.0e9)).solve(t)[0]
    assert (ref["status"] == O.ST_FLIGHT).all()
    assert out.tobytes() == one.tobytes()
    assert (out["status"] == q.ST_FLIGHT).all() and (out["iters"] == 0).all() and np.all(out["u0"][:, 1:] == 0.0)
    assert_parity(q, out, ref, np.ones(9, bool))


@pytest.mark.parametrize("form", FORMS)
def test_all_saturated_beside_a_healthy_group(q, batches, forms, form):
    """HARD 1 (x infeasible: everything saturated after three updates), HARD 13 (y), HARD 6 (both) beside MIX 19 and MIX 0."""
    mix, hard, _, ref_hard = batches
    s, a_mix, a_hard = forms[(form, 8)]
    t = np.concatenate([hard[[1]], mix[[19]], hard[[13]], mix[[0]], hard[[6]]])
    want = np.concatenate([a_hard[[1]], a_mix[[19]], a_hard[[13]], a_mix[[0]], a_hard[[6]]])
    out = s.solve_batch(t)
    check_form(s, form, 8, 5)
    assert out.tobytes() == want.tobytes()
    assert out["status"].tolist() == [q.ST_X_INFEASIBLE, 0, q.ST_Y_INFEASIBLE, 0, q.ST_X_INFEASIBLE | q.ST_Y_INFEASIBLE]
    assert out["status"][[0, 2, 4]].tolist() == ref_hard["status"][[1, 13, 6]].tolist()


# the status a non-finite state carries (the records of these inputs before the masks, every form).  A NaN x runs the tick and returns NaN
# outputs unflagged: the knapsack's compares are all false on NaN, the group leaves the axis at the first count.  An infinite y velocity makes
# |beq| infinite: tau = inf saturates everything, the remainder is infinite, ST_Y_INFEASIBLE after one update (iters 1 | 2 << 8).  A NaN height
# is ST_Z_NAN | ST_FLIGHT (lambda_0 is NaN: flight, never live).
def nonfinite_cases(q):
    """(field, component, value, the status the bad record carries)"""
    return [("com_pos", 0, np.nan, 0), ("com_vel", 1, np.inf, q.ST_Y_INFEASIBLE), ("com_pos", 2, np.nan, q.ST_Z_NAN | q.ST_FLIGHT)]


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_state_beside_a_healthy_group(q, batches, forms, form):
    mix = batches[0]
    s, a_mix, _ = forms[(form, 8)]
    for field, k, v, status in nonfinite_cases(q):
        t = mix[16:24].copy()
        t[field][4, k] = v                                            # MIX 20, between the two instances with four updates
        out = s.solve_batch(t)
        check_form(s, form, 8, 8)
        good = np.arange(8) != 4
        print(f"[{form}] {field}[{k}] = {v}: status {int(out['status'][4])} iters {int(out['iters'][4])}")
        assert out[good].tobytes() == a_mix[16:24][good].tobytes(), (field, k)
        bad = alone(s, t[4:5])
        assert out[4:5].tobytes() == bad.tobytes()
        assert int(out["status"][4]) == status, (field, k, int(out["status"][4]))


# ---- a bound sweep small enough for the 16-lane kernel (SW = 1) ----------------------------------------------------------------------------------
def test_bound_sweep_at_16_lanes(q, batches):
    """8 parameter sets, MIX and HARD interleaved (48 instances, 12 wavefronts of four): unbound, bound, and each instance alone with its set."""
    import torch
    from quadruped_gait_generation_ismpc_amd import workload
    mix, hard = batches[0], batches[1]
    sets = workload.make_sweep_params(8, N=N)
    s = q.MPCSolver.sweep(q.reference_plan(params=sets[0]), sets)
    try:
        t = np.empty(48, dtype=mix.dtype); t[0::2] = mix; t[1::2] = hard
        t["reserved"] = (np.arange(48) * 5 + 3) % 8
        d_in = q.to_device(t)
        a = q.from_device(s.solve_batch_torch(d_in), q.TICK_OUT); torch.cuda.synchronize()
        ia = s.launch_info()
        s.sweep_bind(d_in)
        b = q.from_device(s.solve_batch_torch(d_in), q.TICK_OUT); torch.cuda.synchronize()
        ib = s.launch_info()
        s.sweep_unbind()
        one = alone(s, t)
    finally:
        s.close()
    print(f"sweep launch_info {ia}; bound {ib}")
    for info, bound in ((ia, False), (ib, True)):
        assert (info["lanes"], info["R"], info["sweep"], info["batch"], info["bound_order"]) == (16, 7, True, 48, bound)
    assert a.tobytes() == b.tobytes() and a.tobytes() == one.tobytes()
    itx, ity = iters_xy(a)
    assert ((itx >= 3) & (ity >= 3)).sum() >= 4 and (a["iters"] == 0).sum() >= 4
