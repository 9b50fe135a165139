"""A record does not depend on an instance's wave-mates, nor on where the workgroup boundaries fall.

The per-tick lane-group kernels (ismpc_tick_quad, ismpc_tick_quad_inline, ismpc_tick_quad_one) take their workgroup width per shape
(tick_wpg() in csrc/ismpc_b_group.hpp; quad_launch() sizes the grid from it).  N = 100 at 8 lanes per instance (ISMPC_LPI=8: R = 13,
eight instances per wavefront), batches of 1 .. 257 instances: one lane group, one wavefront, and both sides of every workgroup boundary
of a width of four wavefronts (32 instances) and of one (8 instances).  Per kernel form, the records of a batch are byte-equal to the
records the same handle returns for each of its instances launched alone.  Every fourth instance is lifted (the vertical inequality rows
become active), so the deferred paths of every form run in wavefronts that also hold instances that do not defer.

A sweep handle takes 8 lanes per instance only beyond 8 192 instances (ISMPC_LPI does not change that), so the bound 8-set sweep runs
at 8 193, 8 201 and 8 257 instances -- 1 025, 1 026 and 1 033 wavefronts: the number of workgroups is no multiple of 8 at a width of 1,
2 or 4, which is where sweep_vblock()'s ranges per XCD are of unequal length -- and at the small batches with its 16-lane shape (R = 7).
"""
import numpy as np
import pytest

from test_gpu_dispatch_parity import expected_step, knobs, lift

pytestmark = pytest.mark.gpu

N = 100
BATCHES = [1, 7, 8, 9, 31, 33, 63, 64, 65, 257]
SWEEP_BATCHES_8LANE = [8193, 8201, 8257]
FORMS = ("resident", "two", "one")


@pytest.fixture(scope="module")
def q(built_libs):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import quadruped_gait_generation_ismpc_amd as q
    return q


@pytest.fixture(scope="module")
def cus(q):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def tin():
    """257 instances, every fourth one lifted; a batch of B is its first B."""
    from quadruped_gait_generation_ismpc_amd import workload
    t = workload.make_batch(N, max(BATCHES), seed=4000 + N)
    assert lift(t, N).sum() >= 64
    return t


def make_solver(q, form):
    """The handle of a form, its knobs set before it is created: 8 lanes per instance; `one`: a multi-plan handle with one set and one
    plan forced to one launch (never resident, so it takes ismpc_tick_quad_one at every batch size)."""
    p = q.default_params(N=N)
    plan = q.reference_plan(params=p)
    with knobs(ISMPC_LPI=8, ISMPC_ONE_LAUNCH={"resident": None, "two": 0, "one": 3}[form]):
        return q.MPCSolver.plans([plan], p) if form == "one" else q.MPCSolver(plan, params=p)


def want_info(cus, form, batch):
    w = expected_step(cus, batch, N, lpi=8, one_launch=0 if form == "two" else None, sweep=form == "one")
    if form == "one":          # (expected_step's rule for a handle that is never resident; the handle itself is a multi-plan one, not a sweep)
        w["sweep"] = False; w["plans"] = True
    return w


@pytest.fixture(scope="module")
def forms(q, cus, tin):
    """Per form: the handle, and the record of each of the 257 instances launched ALONE (computed once, never modified)."""
    made = {}
    try:
        for form in FORMS:
            s = make_solver(q, form)
            made[form] = [s, None]
            alone = np.concatenate([s.solve_batch(tin[i:i + 1]) for i in range(len(tin))])
            assert s.launch_info() == want_info(cus, form, 1)
            alone.setflags(write=False)
            made[form][1] = alone
        yield made
    finally:
        for s, _ in made.values():
            s.close()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", FORMS)
def test_batch_records_are_bytewise_the_instances_alone(q, cus, tin, forms, form, batch):
    s, alone = forms[form]
    out = s.solve_batch(tin[:batch])
    info = s.launch_info()
    print(f"launch_info[{form}-{batch}] = {info}")
    assert info == want_info(cus, form, batch)
    assert (info["family"], info["lanes"], info["R"], info["RW"]) == ({"resident": "quad_inline", "two": "quad", "one": "quad_one"}[form], 8, 13, 2)
    act = (out["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    assert ((out["status"] & (q.ST_Z_FAILED | q.ST_BAD_INDEX)) == 0).all()
    lifted = np.arange(batch) % 4 == 1                                 # deferred and undeferred instances side by side in the wavefronts
    assert act.sum() >= 0.75 * lifted.sum() and (~act).sum() >= 0.5 * (~lifted).sum(), (act.sum(), lifted.sum())
    assert out.tobytes() == alone[:batch].tobytes(), np.flatnonzero([out[i].tobytes() != alone[i].tobytes() for i in range(batch)])


def test_forms_agree_bytewise(forms):
    """The multi-plan handle with one set and one plan returns a plain handle's bytes; so does the two-launch form."""
    ref = forms["resident"][1]
    assert forms["one"][1].tobytes() == ref.tobytes()
    assert forms["two"][1].tobytes() == ref.tobytes()


def test_u_traj_at_batch_9(q, cus, tin, forms):
    """The control trajectories of a batch that crosses a wavefront boundary (8 instances) are those of each instance alone."""
    import torch
    s, alone = forms["resident"]
    d_in = q.to_device(tin[:9])
    u = torch.zeros((9, 3 * N), dtype=torch.float64, device=d_in.device)
    out = q.from_device(s.solve_batch_torch(d_in, u_traj=u), q.TICK_OUT)
    torch.cuda.synchronize()
    assert s.launch_info() == want_info(cus, "resident", 9)
    assert out.tobytes() == alone[:9].tobytes()
    for i in range(9):
        u1 = torch.zeros((1, 3 * N), dtype=torch.float64, device=d_in.device)
        s.solve_batch_torch(d_in[i:i + 1].contiguous(), u_traj=u1)
        torch.cuda.synchronize()
        assert u1[0].cpu().numpy().tobytes() == u[i].cpu().numpy().tobytes(), i
    assert torch.isfinite(u).all() and (u[0] != 0).any()


@pytest.fixture(scope="module")
def sweep(q):
    from quadruped_gait_generation_ismpc_amd import workload
    sets = workload.make_sweep_params(8, N=N)
    with knobs(ISMPC_LPI=8):
        s = q.MPCSolver.sweep(q.reference_plan(params=sets[0]), sets)
    t = workload.make_batch(N, max(SWEEP_BATCHES_8LANE), seed=5200)
    lift(t, N)
    t["reserved"] = (np.arange(len(t)) * 5 + 3) % 8          # every wavefront of the unbound launch holds several sets
    yield s, t
    s.close()


@pytest.mark.parametrize("batch", BATCHES + SWEEP_BATCHES_8LANE)
def test_bound_sweep_records_are_bytewise_the_unbound_launch(q, cus, sweep, batch):
    import torch
    s, t = sweep
    d_in = q.to_device(t[:batch])
    s.sweep_unbind()
    a = q.from_device(s.solve_batch_torch(d_in), q.TICK_OUT)
    torch.cuda.synchronize()
    ia = s.launch_info()
    s.sweep_bind(d_in)
    b = q.from_device(s.solve_batch_torch(d_in), q.TICK_OUT)
    torch.cuda.synchronize()
    ib = s.launch_info()
    s.sweep_unbind()
    print(f"launch_info[sweep-{batch}] = {ia}; bound = {ib}")
    lanes = 8 if batch > 8192 else 16
    # (a handle that has seen a deferral takes the two-launch form for its next launches: the rule of launch(), not of a fresh handle)
    for info, bound in ((ia, False), (ib, True)):
        want = expected_step(cus, batch, N, sweep=True, bound=bound)
        assert (info["lanes"], info["R"], info["RW"], info["sweep"], info["batch"], info["bound_order"]) == (lanes, want["R"], 2, True, batch, bound)
        assert (info["family"], info["kernels"]) in (("quad_one", 1), ("quad", 2))
    assert want["lanes"] == lanes
    assert ((a["status"] & (q.ST_Z_FAILED | q.ST_BAD_INDEX)) == 0).all()
    if batch >= 8:                                             # the deferred paths did run (how many of the lifted instances defer depends on their set)
        assert ((a["status"] & q.ST_Z_INEQ_ACTIVE) != 0).any() and ((a["status"] & q.ST_Z_INEQ_ACTIVE) == 0).any()
    assert a.tobytes() == b.tobytes()
