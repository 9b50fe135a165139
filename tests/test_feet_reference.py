"""The swing-foot re-placement (the scripts' second quadprog) on the CPU: the independent reference of tests/helpers/feet_reference.py
-- the QP solved as a QP, by enumeration of its active sets, on a target computed in long double -- against the oracle's closed-form
foot step (oracle/ismpc_oracle_a.c, orc_a_foot_step), on the very inputs that tests/test_gpu_formulation_a_feet.py gives the device.

The coverage conditions of those inputs (every constraint row active in >= 10 % of the QPs, >= 10 % of the QPs free, both parities,
all four walking feet, a first step decided by its halved limits, the fc = 8 write-back) are asserted here from the reference alone;
the offset scales of tests/helpers/feet_cases.py were chosen with this file.  The largest deviation of the plain-C fp64 oracle from the
reference over these inputs, feet_cases.DEV_ORACLE, is what the device tests take their tolerance from (8 times it).

With the lateral limits of the even trot steps as they were before this file existed (BR given the left feet's interval, FL the right
feet's) the even-fc instances of every trot case here differ from the reference by centimetres: disp_i != disp_o shows it."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle_a as A

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("feet_cases", os.path.join(HERE, "helpers", "feet_cases.py"))
F = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(F)
R = F.R

DEV_CORE = DEV_LOOP = F.DEV_ORACLE      # the closed loop is held to the core inputs' figure (feet_cases.py)
LOOP_TICKS = F.LOOP_TICKS
oracle_for, oracle_steps = F.oracle_for, F.oracle_steps


def case_z(name, case):
    """The predicted footsteps the CPU tests feed: the oracle's own, moved by a seeded centimetre in the id that pushes."""
    push = F.CASES[name].get("push")
    return case["f0"] + (np.random.default_rng(99).uniform(-0.5, 0.5, case["f0"].shape) * push if push else 0.0)


def test_enumeration_does_not_assume_a_box(built_libs):
    X, act = R.solve_qp(np.array([2.0, 2.0]), np.array([[1.0, 1.0], [1.0, 0.0], [-1.0, 0.0]]), np.array([1.0, 5.0, 5.0]))
    assert np.abs(X - 0.5).max() <= 1e-15 and act.tolist() == [True, False, False]
    X, act = R.solve_qp(np.array([3.0, 0.0]), np.array([[1.0, 1.0], [1.0, -1.0]]), np.array([1.0, 1.0]))      # a vertex
    assert np.abs(X - [1.0, 0.0]).max() <= 1e-15 and act.all()
    X, act = R.solve_qp(np.array([0.2, -0.1]), np.array([[0.0, 1.0], [0.0, -1.0], [1.0, 0.0]]), np.array([1.0, 1.0, 1.0]))
    assert (X == [0.2, -0.1]).all() and not act.any()


@pytest.mark.parametrize("cfg", sorted(F.CONFIGS))
def test_states_fixture_is_the_oracles_closed_loop(cfg, built_libs):
    """tests/golden/feetA_states.npz holds what the oracle's unpushed closed loop gives today: fc covers 1 .. 10, twice each."""
    st, f0 = F.harvest(*F.CONFIGS[cfg])
    st2, f02 = F.harvest_from_oracle(*F.CONFIGS[cfg])
    assert sorted(st["fc"].tolist()) == sorted(list(F.FCS) * 2)
    for k in ("fc", "j", "rebuilt", "reserved"):
        assert (st[k] == st2[k]).all()
    for k in ("x", "xd", "xz", "y", "yd", "yz", "cur_x", "cur_y", "off_x", "off_y"):
        assert np.abs(st[k] - st2[k]).max() <= 1e-9, k
    assert np.abs(f0 - f02).max() <= 1e-9


@pytest.mark.parametrize("name", sorted(F.CASES))
def test_reference_against_oracle_foot_step(name, built_libs):
    case = F.build(name)
    z = case_z(name, case)
    ref, active = F.reference(case, z)
    counts = F.coverage(case, active)                                   # the coverage conditions, from the reference alone
    orc, ran = oracle_steps(case, z)
    assert ran.all()
    err, ties = F.errors(case, z, orc, ref, active)
    dev = err.max()
    moved = np.abs(ref - case["plans"]).reshape(len(ran), -1).max(1) > 1e-6
    print("FEET", name, "oracle-vs-reference", dev, "ties", ties, "coverage", counts, "instances moved", int(moved.sum()))
    assert dev <= DEV_CORE, dev
    assert moved.sum() == sum(a is not None for a in active)            # every QP instance did change its plan, no other did


@pytest.mark.parametrize("name", sorted(F.EOP_CASES))
def test_end_of_plan_rule(name, built_libs):
    """A plan truncated to a few rows, states with fc on either side of `re-place iff 1 <= fc <= rows - 1` (include/ismpc_a.h)."""
    case = F.build_eop(name)
    cfg, rows, (last, first_not) = F.EOP_CASES[name]
    assert case["plans"].shape[1] == rows + R.FEET_PAD and set(case["fc"].tolist()) == {last, first_not}
    assert R.replaces(last, rows) and not R.replaces(first_not, rows) and not R.replaces(rows, rows) and R.replaces(rows - 1, rows)
    ref, active = F.reference_with_rule(case, case["f0"])
    orc, ran = oracle_steps(case, case["f0"])
    assert (ran == (case["fc"] == last)).all()
    assert F.errors(case, case["f0"], orc, ref, active)[0].max() <= DEV_CORE
    stay = case["fc"] == first_not
    assert stay.any() and (orc[stay] == case["plans"][stay]).all() and (ref[stay] == case["plans"][stay]).all()
    assert all(a is not None for a, s in zip(active, stay) if not s)
    assert (np.abs(orc[~stay] - case["plans"][~stay]).reshape((~stay).sum(), -1).max(1) > 1e-6).all()   # the last fc does re-place


@pytest.mark.parametrize("cfg", ["trot_phipi4", "walk_phipi4"])
def test_closed_loop_reference_against_oracle(cfg, built_libs):
    """400 ticks of the oracle's closed loop with the small unequal limits; every tick's foot step against feet_step on the
    oracle's own plan before the tick and its own predicted footstep."""
    kind, phi = F.CONFIGS[cfg]
    sim = oracle_for(kind, phi)
    lim = F.LIMITS
    dev, steps, bounded, ties = 0.0, 0, 0, 0
    for t in range(LOOP_TICKS):
        before = sim.foot_plan_padded()
        r = sim.tick()
        assert r["rv"][0] == 0 and r["rv"][1] == 0
        e, _, act, tie = R.step_error(sim.foot_plan_padded(), kind, phi, lim["disp_i"], lim["disp_o"], lim["disp_forw"], int(r["fc"]), r["f0"], before)
        dev = max(dev, e)
        if act is not None:
            steps += 1; bounded += bool(act.any()); ties += tie
    print("FEET loop", cfg, "oracle-vs-reference", dev, "foot steps", steps, "with an active bound", bounded, "ties of d != 0", ties)
    assert dev <= DEV_LOOP, dev
    assert steps >= LOOP_TICKS // 4 and bounded >= 0.10 * steps


def test_a_footstep_on_the_fixed_diagonal_is_a_tie(built_libs):
    """The scripts re-place the feet `if d != 0`.  A predicted footstep that the tick's QP pins to the fixed diagonal has d = 0 up to
    the rounding of z.  This z is the device's out.f0 of instance 221 of trot_phipi4_push_b257 (fc = 1): d = 1.5e-18 m in long double.
    The reference decides as the scripts do, on the exact intersection rounded to double -- unchanged, as the oracle finds in plain
    fp64 -- and marks the step a tie; a nanometre off the diagonal it is no tie."""
    case = F.build("trot_phipi4_push_b257")
    kind, phi, plan = case["kind"], case["phi"], case["plans"][221]
    assert case["fc"][221] == 1
    z = (float.fromhex("0x1.f35e17484cf37p-2"), float.fromhex("0x1.cc60a9ca79400p-6"))
    d, _, changed, tie, _, _ = R.displacement(kind, 1, z, plan)
    assert tie and not changed and 0 < max(abs(d[0]), abs(d[1])) < 1e-17
    lim = F.LIMITS
    sim = oracle_for(kind, phi); sim.set_foot_plan_padded(plan); assert sim.foot_step(1, z)
    e, ref, act, tie = R.step_error(sim.foot_plan_padded(), kind, phi, lim["disp_i"], lim["disp_o"], lim["disp_forw"], 1, z, plan)
    assert tie and e <= DEV_CORE and act is not None
    d, _, changed, tie, _, _ = R.displacement(kind, 1, (z[0], z[1] + 1e-9), plan)
    assert changed and not tie
