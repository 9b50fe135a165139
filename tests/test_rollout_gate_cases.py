"""The preconditions of tests/test_gpu_rollout_gates.py, asserted on the CPU oracle alone (tests/helpers/rollout_gate_cases.py), so that
they are checked wherever the suite runs: the frame table of every scenario, the identity of a continued oracle rollout with the uncut
one, the error-free run up to the end of the plan, the oracle's statuses around the NaN guard, and the restated caller bookkeeping
against the oracle's own rollout."""
import numpy as np
import pytest

from helpers import rollout_gate_cases as G
from oracle import oracle as O


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()


@pytest.mark.parametrize("name", list(G.SCENARIOS))
def test_frame_table(name):
    """nmid, the last tick that runs, the first BAD_INDEX tick; every tick behind it that is not skipped is BAD_INDEX and nothing else,
    and the skip test comes first (divisor 2: the tail alternates 32, 8)."""
    sc = G.SCENARIOS[name]
    orc = G.make_oracle(name)
    assert len(orc.midpoint()) == sc["nmid"] == sc["rows"] * G.S_F
    st = G.scenario(name)["outs"]["status"]
    assert st.shape == (sc["ticks"], G.B)
    for i in range(G.B):                                            # integer decisions: the same frames on every instance
        ran = np.flatnonzero((st[:, i] & G.GATE_BITS) == 0)
        bad = np.flatnonzero((st[:, i] & O.ST_BAD_INDEX) != 0)
        assert ran[-1] == sc["last_run"] and bad[0] == sc["first_bad"], (name, i, ran[-1], bad[0])
    tail = st[sc["first_bad"]:]
    divisor = int(100 * sc["mpc_dt"])
    if divisor == 1:
        assert (tail == O.ST_BAD_INDEX).all() and ((st & O.ST_TICK_SKIPPED) == 0).all()
    else:
        assert divisor == 2 and set(np.unique(tail)) == {O.ST_BAD_INDEX, O.ST_TICK_SKIPPED}
        assert (tail[0::2, 0] == O.ST_BAD_INDEX).all() and (tail[1::2, 0] == O.ST_TICK_SKIPPED).all(), tail[:, 0]
        assert st[sc["last_run"] + 1, 0] == O.ST_TICK_SKIPPED
        skipped = (st[:sc["first_bad"]] & O.ST_TICK_SKIPPED) != 0
        assert 0.4 < skipped.mean() < 0.6                            # every second tick, up to the counter resets at a step
    counts = {int(v): int((st[sc["start"]:, 0] == v).sum()) for v in np.unique(st[sc["start"]:, 0])}
    print(f"{name}: nominal instance, ticks {sc['start']}..{sc['ticks'] - 1} by status {counts}")


@pytest.mark.parametrize("name", list(G.SCENARIOS))
def test_oracle_is_clean_up_to_the_end_of_the_plan(name):
    """At least 12 of the 13 instances carry no error bit before the first BAD_INDEX tick, the nominal one among them, and no tick carries
    Z_FAILED.  (Tried when the scenarios were chosen: all 13 are clean in every scenario.)"""
    upto = G.compare_upto(name)
    print(f"{name}: instances compared to the end {int((upto == G.SCENARIOS[name]['ticks']).sum())} of {G.B}")


@pytest.mark.parametrize("name", ["gate100", "gate50"])
def test_continuation_is_the_uncut_rollout(name):
    """Oracle.rollout from its own final state after `start` ticks, at first_frame = start, is the uncut rollout: records and final state,
    byte for byte.  (Restarting from ins[start] is not: that record already has the bookkeeping of tick `start` applied.)"""
    sc, d = G.SCENARIOS[name], G.scenario(name)
    orc = G.make_oracle(name)
    for i in (0, 5, 12):
        outs, ins, _, fin = orc.rollout(d["recs"][i:i + 1], 0, sc["ticks"])
        assert outs.tobytes() == d["outs"][:, i].tobytes() and ins.tobytes() == d["ins"][:, i].tobytes(), (name, i)
        assert fin.tobytes() == d["fin"][i:i + 1].tobytes()
    assert d["start_state"]["control_iter"].max() > 0 and (d["start_state"]["simulation_time"] == sc["start"] - 1).all()


def test_final_counters_of_the_nominal_instance():
    fin = G.scenario("end100")["fin"]
    assert (fin["control_iter"][0], fin["mpc_iter"][0], fin["footstep_counter"][0]) == (37, 37, 6)
    assert fin["simulation_time"][0] == G.SCENARIOS["end100"]["ticks"] - 1


@pytest.mark.parametrize("name", ["end50", "gate50"])
def test_restated_bookkeeping_is_the_oracles(name):
    """caller_loop (the bookkeeping of Controller.cpp:297-304, :310, :346-348, :503-504 restated in numpy) around the oracle's single
    tick is the oracle's own rollout, byte for byte: what the GPU test drives around ismpc_solve_batch is the loop the oracle runs."""
    sc, d = G.SCENARIOS[name], G.scenario(name)
    orc = G.make_oracle(name)
    k = sc["ticks"] - 60
    start = orc.rollout(d["recs"][0:1], 0, k)[3]
    two = np.concatenate([start, start])
    traj, fin = G.caller_loop(lambda r: orc.solve(r)[0], two, orc.ftsp, orc.params.control_dt, orc.params.mpc_dt, k, 60)
    for j in range(2):
        assert np.stack(traj)[:, j].tobytes() == d["outs"][k:, 0].tobytes()
        assert fin[j:j + 1].tobytes() == d["fin"][0:1].tobytes()


def test_nan_guard_statuses():
    """nan100 on the oracle (backend gi): the poisoned tick is ST_Z_NAN | ST_FLIGHT with z = h_des exactly and zd = +0; every later tick
    has status 0, a finite z (0.6817 after 40 ticks) and NaN in x and y; the healthy instances do not notice."""
    n = G.nan_case()
    h_des = G.oracle_params("end100").h_des
    for outs, t0, who in ((n["outs"], 0, G.NAN_Z + G.NAN_ZD), (n["mc_outs"], G.NAN_CLEAN, G.NAN_Z + G.NAN_ZD)):
        for i in who:
            g = outs[t0, i]
            assert g["status"] == (O.ST_Z_NAN | O.ST_FLIGHT) == 80
            assert g["com_pos"][2].tobytes() == np.float64(h_des).tobytes() and g["com_vel"][2].tobytes() == np.float64(0.0).tobytes()
            later = outs[t0 + 1:, i]
            assert (later["status"] == 0).all()
            assert np.isfinite(later["com_pos"][:, 2]).all() and np.isfinite(later["com_vel"][:, 2]).all()
            assert abs(later["com_pos"][-1, 2] - 0.6817) < 5e-5
            assert np.isnan(outs[t0:, i]["com_pos"][:, :2]).all() and np.isnan(outs[t0:, i]["com_vel"][:, :2]).all()
        healthy = [i for i in range(G.B) if i not in who]
        assert (outs["status"][:, healthy] & ~O.ST_FLIGHT).sum() == 0 and np.isfinite(outs["com_pos"][:, healthy]).all()
    healthy = [i for i in range(G.B) if i not in G.NAN_Z + G.NAN_ZD]
    assert n["outs"][:, healthy].tobytes() == n["healthy_outs"][:, healthy].tobytes()


def test_failed_vertical_solve_on_the_oracle():
    z = G.zfail_case()
    assert ((z["first_tick"]["status"] & O.ST_Z_FAILED) != 0).all()
