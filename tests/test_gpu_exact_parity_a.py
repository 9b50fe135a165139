"""Formulation A kernels against one tick in exact arithmetic (tests/helpers/exact_tick_a.py, fixtures tests/golden/formA_exact_*.npz), at
rounding level: DESIGN.md 3.2.

fp64: every quantity of every tick within 16 x the group's stored floor (the larger of the fp64 oracle's and a plain numpy KKT solve's
error against the same exact values, cur / off at least the f0 error; 16 = four bits for summation order and table precision, as in 3.1), status, fc, j and rebuilt bit
for bit, nothing excluded, iters_* not compared.  Forms: the default wave kernel, the workgroup kernel (ISMPC_A_KERNEL=block; plain
handles only: a per-instance batch always runs the wave kernel), cold starts (ISMPC_A_WARM=0), the working-set history off
(ISMPC_A_HISTORY=0) and on (ismpc_a_set_warm_history: the tick is run twice, the second time from the working set the first ended on),
one launch per footstep count (ISMPC_A_BUCKET 0 | 1, per-instance group).  The two closed loops go through the on-device rollout (the
prefix before the first push through ismpc_a_rollout_device, the whole loop with its pushes through ismpc_a_rollout_mc_device) and through
the caller-driven tick loop with warm history.

out.active is compared with the certified working-set sizes under the kernels' own counting convention (ismpc_a_wave.hpp: q = 1 + qz + qk,
ismpc_a_block.hpp: q starts at 1 with the stability row): the stability row counts, then every active ZMP row and every active kinematic
row; x in the low 16 bits, y in the high ones.  The fixtures' ticks have a slack margin >= 1e-8 m and a multiplier margin >= 1e-6, five
orders above the fp64 violation threshold, so another working set is a wrong answer.

fp32 (precision="f32", ISMPC_A_F32_RESOLVE on and off): single ticks only (tests/test_gpu_formulation_a_edges.py says why no fp32 loop
bound exists), against the exact values, within 16 x 2^29 x the fp64 floor -- the ratio of the unit roundoffs; the condition-number
amplification is the same in both precisions -- and, additionally, within the bounds the existing fp32 tests hold (next CoM 1e-6 relative,
velocity 5e-6, f0 2e-5, u0 2e-3), so nothing gets looser.  With floors set by an ill-conditioned plain KKT solve the 2^29 bound comes out
at 1e-2 .. 1e-1 m/s for u0: the fp32 side of this file is NOT a net at rounding level, it is a second set of shapes under the held bounds
(DESIGN.md 3.2 has the measured figures).  Every measured maximum goes through _record_maxima."""
import numpy as np
import pytest

from helpers import exact_tick_a as X
from test_gpu_formulation_a import _record_maxima, q_from_dev, q_to_dev

pytestmark = pytest.mark.gpu

KNOBS = ("ISMPC_A_KERNEL", "ISMPC_A_BUCKET", "ISMPC_A_CLAIM", "ISMPC_A_STATIC", "ISMPC_A_PRECISION", "ISMPC_A_WARM", "ISMPC_A_HISTORY", "ISMPC_A_F32_RESOLVE")
PLAIN_GROUPS = ("walk_C100", "trot_C160", "edges")
LOOP_GROUPS = ("loop_walk_C100", "loop_trot_C65")
FORMS = {"wave": {}, "block": {"ISMPC_A_KERNEL": "block"}, "cold": {"ISMPC_A_WARM": "0"}, "nohist": {"ISMPC_A_HISTORY": "0"}, "hist": {}}
F32_FORMS = {"resolve": {}, "noresolve": {"ISMPC_A_F32_RESOLVE": "0"}}


@pytest.fixture(scope="module")
def FA(built_libs):
    import torch
    assert torch.cuda.is_available()
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    return FA


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def on_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def handle(FA, fx, case, precision="f64", plans=(0,)):
    """A handle with exactly the fixture's parameters; plans: indices into the fixture's base plans, the first given to ismpc_a_create."""
    row = fx["params"][case]
    p = FA.default_params(FA.TROT)
    for k, v in zip(X.PARAM_FIELDS, row):
        setattr(p, k, int(v) if k in X.INT_FIELDS else float(v))
    gen = FA.GaitGenerator(p, np.array(fx["centers"][plans[0]]), precision=precision)
    for k, pl in enumerate(plans[1:], 1):
        assert gen.add_plan(np.array(fx["centers"][pl])) == k
    return gen


def run_single_ticks(FA, fx, precision, hist):
    """Every tick of a single-tick fixture through its case's handle: (OUT_A [n], STATE_A after [n])."""
    n = len(fx["case"])
    out, after = np.zeros(n, FA.OUT_A), np.zeros(n, FA.STATE_A)
    states = fx["state"].view(FA.STATE_A).reshape(-1)
    for case in range(len(fx["params"])):
        sel = np.flatnonzero(fx["case"] == case)
        plan = int(fx["plan"][sel[0]])
        if fx["has_inst"]:
            gen = handle(FA, fx, case, precision, plans=(0, 1))                     # trot, walk: what inst.plan indexes
            inst = q_to_dev(fx["inst"][sel].view(FA.INST_A).reshape(-1).copy())
            tick = lambda d, p: gen.tick_inst_torch(d, inst, p)
        else:
            assert (fx["plan"][sel] == plan).all()
            gen = handle(FA, fx, case, precision, plans=(plan,))
            tick = gen.tick_torch
        push = on_dev(fx["push"][sel])
        if hist:
            gen.set_warm_history(True)
            first = q_from_dev(tick(q_to_dev(states[sel].copy()), push), FA.OUT_A)
        d = q_to_dev(states[sel].copy())
        out[sel] = q_from_dev(tick(d, push), FA.OUT_A)
        after[sel] = q_from_dev(d, FA.STATE_A)
        if hist:
            assert np.array_equal(first["status"], out["status"][sel]) and np.array_equal(first["active"], out["active"][sel])
        gen.close()
    return out, after


def check_fp64(fx, out, after, label):
    exact = X.fixture_exact(fx)
    fl = X.group_floor(fx)
    e = X.assert_exact_a(X.quantities(out, after), exact, fl, X.BOUND_FACTOR, label=label, same_input=not fx["loop"])
    assert np.array_equal(X.active_sizes(out), X.active_sizes(fx["out"].view(X.OUT_A).reshape(-1))), (label, X.active_sizes(out).tolist())
    _record_maxima(f"exactA:{label}", dict(**e, **{f"ratio_{k}": e[k] / fl[k] for k in X.QUANTITIES}))
    return e


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("group", PLAIN_GROUPS)
def test_single_ticks_fp64(FA, group, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    fx = X.load_group(group)
    out, after = run_single_ticks(FA, fx, "f64", hist=form == "hist")
    check_fp64(fx, out, after, f"{group}:{form}")


@pytest.mark.parametrize("bucket", [0, 1])
@pytest.mark.parametrize("form", ["wave", "cold", "nohist", "hist"])
def test_per_instance_ticks_fp64(FA, form, bucket, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ISMPC_A_BUCKET", str(bucket))
    fx = X.load_group("inst_C200")
    out, after = run_single_ticks(FA, fx, "f64", hist=form == "hist")
    check_fp64(fx, out, after, f"inst_C200:{form}:bucket{bucket}")


# ---- the two closed loops -------------------------------------------------------------------------------------------------------------------
def rollout_view(q, last_only=("zmp", "cur_off", "fc", "j", "rebuilt")):
    """What a trajectory of OUT_A records and the final state show of quantities(): u0, f0, vel_after and status of every tick, the next
    CoM of every tick (com_before of the following one; the final state's for the last), everything else of the last tick."""
    v = dict(q)
    v["vel"] = q["vel"][:, :2]
    for k in last_only:
        v[k] = q[k][-1:]
    return v


def traj_quantities(traj, final):
    n = len(traj)
    st = np.zeros(n, X.STATE_A)
    st["x"][:-1], st["y"][:-1] = traj["com_before"][1:, 0], traj["com_before"][1:, 1]
    st[-1] = final
    st["xd"], st["yd"] = traj["vel_after"][:, 0], traj["vel_after"][:, 1]
    return rollout_view(X.quantities(traj, st))


def check_loop(fx, got, label, ticks=None):
    exact = X.fixture_exact(fx, None if ticks is None else np.arange(ticks))
    fl = X.group_floor(fx)
    e = X.assert_exact_a(got, rollout_view(exact), fl, X.BOUND_FACTOR, label=label, same_input=False)
    _record_maxima(f"exactA:{label}", dict(**e, **{f"ratio_{k}": e[k] / fl[k] for k in X.QUANTITIES}))


@pytest.mark.parametrize("form", ["wave", "block", "cold", "nohist"])
@pytest.mark.parametrize("group", LOOP_GROUPS)
def test_closed_loop_on_device_fp64(FA, group, form, monkeypatch):
    """ismpc_a_rollout_device up to the first push, ismpc_a_rollout_mc_device with the push table over the whole loop; two identical
    instances must give identical bytes."""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    fx = X.load_group(group)
    n = len(fx["case"])
    s0 = np.repeat(fx["state"][:1].view(FA.STATE_A).reshape(-1), 2)
    pushed = np.flatnonzero(np.abs(fx["push"]).max(1) > 0)
    want_active = X.active_sizes(fx["out"].view(X.OUT_A).reshape(-1))
    gen = handle(FA, fx, 0, plans=(int(fx["plan"][0]),))
    st = q_to_dev(s0.copy())
    pre = q_from_dev(gen.rollout_torch(st, int(pushed[0])), FA.OUT_A)
    fin = q_from_dev(st, FA.STATE_A)
    gen.close()
    assert pre[:, 0].tobytes() == pre[:, 1].tobytes() and fin[0].tobytes() == fin[1].tobytes()
    check_loop(fx, traj_quantities(pre[:, 0], fin[0]), f"{group}:{form}:rollout_prefix", ticks=int(pushed[0]))
    assert np.array_equal(X.active_sizes(pre[:, 0]), want_active[:pushed[0]])
    table = np.zeros((2, len(pushed)), FA.PUSH_A)
    table["tick"], table["dv"] = pushed[None, :], fx["push"][pushed][None, :, :]
    gen = handle(FA, fx, 0, plans=(int(fx["plan"][0]),))
    st = q_to_dev(s0.copy())
    traj, _ = gen.rollout_mc_torch(st, n, pushes=q_to_dev(table).reshape(2, len(pushed), 24), want_summary=False)
    traj, fin = q_from_dev(traj, FA.OUT_A), q_from_dev(st, FA.STATE_A)
    gen.close()
    assert traj[:, 0].tobytes() == traj[:, 1].tobytes() and fin[0].tobytes() == fin[1].tobytes()
    check_loop(fx, traj_quantities(traj[:, 0], fin[0]), f"{group}:{form}:rollout_mc")
    assert np.array_equal(X.active_sizes(traj[:, 0]), want_active)


@pytest.mark.parametrize("form", ["wave", "block", "nohist"])
@pytest.mark.parametrize("group", LOOP_GROUPS)
def test_closed_loop_caller_driven_fp64(FA, group, form, monkeypatch):
    """ismpc_a_set_warm_history(h, 1), then one ismpc_a_tick_batch_device call per tick with the tick's push: the state after EVERY tick."""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    fx = X.load_group(group)
    n = len(fx["case"])
    gen = handle(FA, fx, 0, plans=(int(fx["plan"][0]),))
    gen.set_warm_history(True)
    st = q_to_dev(fx["state"][:1].view(FA.STATE_A).reshape(-1).copy())
    out, after = np.zeros(n, FA.OUT_A), np.zeros(n, FA.STATE_A)
    for t in range(n):
        out[t] = q_from_dev(gen.tick_torch(st, on_dev(fx["push"][t:t + 1])), FA.OUT_A)[0]
        after[t] = q_from_dev(st, FA.STATE_A)[0]
    gen.close()
    check_fp64(fx, out, after, f"{group}:{form}:tick_loop")


# ---- fp32 ---------------------------------------------------------------------------------------------------------------------------------
def check_fp32(fx, out, after, label):
    exact = X.fixture_exact(fx)
    got = X.quantities(out, after)
    fl = {k: v * X.F32_RATIO for k, v in X.group_floor(fx).items()}
    held = dict(com=float((np.abs(got["com"] - exact["com"]) / np.maximum(np.abs(exact["com"]), 1e-3)).max()),
                vel=float(np.abs(got["vel"] - exact["vel"]).max()), f0=float(np.abs(got["f0"] - exact["f0"]).max()),
                u0=float((np.abs(got["u0"] - exact["u0"]) / np.maximum(1.0, np.abs(exact["u0"]))).max()))
    e = X.errors(got, exact)
    _record_maxima(f"exactA32:{label}", dict(**e, **{f"ratio_{k}": e[k] / fl[k] for k in X.QUANTITIES}, **{f"held_{k}": v for k, v in held.items()}))
    X.assert_exact_a(got, exact, fl, X.BOUND_FACTOR, label=label)
    assert held["com"] <= 1e-6 and held["vel"] <= 5e-6 and held["f0"] <= 2e-5 and held["u0"] <= 2e-3, (label, held)


@pytest.mark.parametrize("form", list(F32_FORMS))
@pytest.mark.parametrize("group", PLAIN_GROUPS)
def test_single_ticks_fp32(FA, group, form, monkeypatch):
    for k, v in F32_FORMS[form].items():
        monkeypatch.setenv(k, v)
    fx = X.load_group(group)
    out, after = run_single_ticks(FA, fx, "f32", hist=False)
    check_fp32(fx, out, after, f"{group}:{form}")


@pytest.mark.parametrize("bucket", [0, 1])
@pytest.mark.parametrize("form", list(F32_FORMS))
def test_per_instance_ticks_fp32(FA, form, bucket, monkeypatch):
    for k, v in F32_FORMS[form].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("ISMPC_A_BUCKET", str(bucket))
    fx = X.load_group("inst_C200")
    out, after = run_single_ticks(FA, fx, "f32", hist=False)
    check_fp32(fx, out, after, f"inst_C200:{form}:bucket{bucket}")
