"""Scenarios for closed loops at ticks that do NOT run (tests/test_rollout_gate_cases.py, tests/test_gpu_rollout_gates.py): gated ticks
(mpc_dt = 2 control_dt), the end of the footstep plan inside a rollout, the NaN guard inside a loop and a vertical solve that fails on
every tick.  Everything here is numpy and the CPU oracle (backend "gi", named explicitly: its statuses on NaN data are known); nothing
imports the GPU package.  Every oracle result is computed once per process, shared and read-only.

Small plans, so that the plan ends after a few hundred ticks.  With rows plan rows the midpoint table has nmid = rows (S + F) rows; tick
`frame` reads the window [idx, idx + 2N) with idx = (int)(frame / (mpc_dt / control_dt)), so the last frame that runs has
idx = nmid - 2N and every later one that is not skipped (the skip test comes first) is ISMPC_ST_BAD_INDEX.
"""
import numpy as np

from oracle import oracle as O

B = 13                           # a partial last wavefront at 8, 16 and 32 lanes per instance
S_F = 45                         # S + F of the reference's gait timing
# name: N, plan rows, mpc_dt, nmid, last tick that runs, first BAD_INDEX tick, ticks, start (the device runs of the gate* scenarios
# continue the oracle's own state after `start` ticks, about 150 ticks before the end)
SCENARIOS = {
    "end100":  dict(N=100, rows=10, mpc_dt=0.01, nmid=450, last_run=250, first_bad=251, ticks=262, start=0),
    "end50":   dict(N=50,  rows=8,  mpc_dt=0.01, nmid=360, last_run=260, first_bad=261, ticks=272, start=0),
    "end150":  dict(N=150, rows=14, mpc_dt=0.01, nmid=630, last_run=330, first_bad=331, ticks=342, start=0),
    "gate100": dict(N=100, rows=14, mpc_dt=0.02, nmid=630, last_run=860, first_bad=862, ticks=873, start=723),
    "gate50":  dict(N=50,  rows=10, mpc_dt=0.02, nmid=450, last_run=700, first_bad=702, ticks=713, start=563),
}
GATE_BITS = O.ST_TICK_SKIPPED | O.ST_BAD_INDEX
QP_ERRORS = O.ST_X_INFEASIBLE | O.ST_Y_INFEASIBLE | O.ST_Z_FAILED

NAN_CLEAN, NAN_TICKS = 30, 40    # nan100: 30 clean ticks, then 40 from the poisoned state
NAN_Z, NAN_ZD = (3, 11), (7,)    # instances with com_pos[2] = NaN | com_vel[2] = NaN
ZFAIL_LO, ZFAIL_TICKS = 1e-3, 8  # z_ineq_lo of tests/test_gpu_padding.py: S u is 0 at sample 0, a bound above zero cannot be met

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def oracle_params(name, **over):
    sc = SCENARIOS[name]
    return O.default_params(sc["N"], mpc_dt=sc["mpc_dt"], **over)


def plan(name):
    sc = SCENARIOS[name]
    return O.reference_plan(rows=sc["rows"], mpc_dt=sc["mpc_dt"])


def make_oracle(name, **over):
    return O.Oracle(oracle_params(name, **over), plan(name), backend="gi")


def initial_records():
    """Instance 0 is the reference's initial state; the other twelve are perturbed by +-0.002 m in x, y and +-0.01 m/s in the
    horizontal velocity."""
    recs = np.repeat(O.initial_state(), B)
    rng = np.random.default_rng(5)
    recs["com_pos"][1:, :2] += rng.uniform(-0.002, 0.002, (B - 1, 2))
    recs["com_vel"][1:, :2] += rng.uniform(-0.01, 0.01, (B - 1, 2))
    return recs


def rollout_all(orc, recs, first_frame, ticks):
    """Oracle.rollout per instance: (outs [ticks, B], ins [ticks, B], final states [B])."""
    outs = np.zeros((ticks, len(recs)), dtype=O.TICK_OUT); ins = np.zeros((ticks, len(recs)), dtype=O.TICK_IN)
    fin = np.zeros(len(recs), dtype=O.TICK_IN)
    for i in range(len(recs)):
        o, n, _, f = orc.rollout(recs[i:i + 1], first_frame, ticks)
        outs[:, i] = o; ins[:, i] = n; fin[i] = f[0]
    return outs, ins, fin


def scenario(name):
    """The oracle side of an end* / gate* scenario: dict(recs, start_state, outs, ins, fin) -- outs and ins are [ticks, B] over the WHOLE
    run from frame 0 (computed in two cuts: frames [0, start) and [start, ticks), the second from the final state of the first -- what
    the device continues from); start_state is the state after `start` ticks (the initial records when start = 0)."""
    def make():
        sc = SCENARIOS[name]
        orc = make_oracle(name)
        recs = initial_records()
        k, ticks = sc["start"], sc["ticks"]
        if k:
            o1, i1, mid = rollout_all(orc, recs, 0, k)
            o2, i2, fin = rollout_all(orc, mid, k, ticks - k)
            outs, ins = np.concatenate([o1, o2]), np.concatenate([i1, i2])
        else:
            mid = recs.copy()
            outs, ins, fin = rollout_all(orc, recs, 0, ticks)
        frozen(recs, mid, outs, ins, fin)
        return dict(recs=recs, start_state=mid, outs=outs, ins=ins, fin=fin)
    return cached(("scenario", name), make)


def compare_upto(name):
    """Assertion 1 of the issue, from the oracle alone: per instance the first tick with an oracle error bit before the first BAD_INDEX
    tick (`ticks` when there is none: compared to the end).  At most one instance may have one, and never the nominal instance; a tick
    that does run never carries Z_FAILED (the oracle feeds a failed tick back, the device does not: no reference behind it)."""
    sc, st = SCENARIOS[name], scenario(name)["outs"]["status"]
    assert ((st & O.ST_Z_FAILED) == 0).all(), (name, "Z_FAILED in the oracle's run")
    err = (st[:sc["first_bad"]] & O.ST_ERROR_MASK) != 0
    upto = np.where(err.any(axis=0), err.argmax(axis=0), sc["ticks"])
    dirty = np.flatnonzero(upto < sc["ticks"])
    assert len(dirty) <= 1, (name, "instances with an oracle error bit before the end of the plan", dirty, upto[dirty])
    assert upto[0] == sc["ticks"], (name, "the nominal instance is not clean", upto[0])
    return upto


# ---- nan100 --------------------------------------------------------------------------------------------------------------------------
def nan_case():
    """end100's plan and parameters.  dict(clean: the oracle's states after 30 clean ticks, poisoned: the same with com_pos[2] = NaN on
    instances 3 and 11 and com_vel[2] = NaN on 7, outs / fin: the oracle's 40 ticks from `poisoned` at first_frame 30, healthy_outs: the
    same from `clean`; mc_*: the rollout the disturbed loop reaches from inside -- com_vel[2] += NaN on instances 3, 7 and 11 in front
    of tick 30 of 70 ticks from the initial records)."""
    def make():
        orc = make_oracle("end100")
        recs = initial_records()
        o0, _, clean = rollout_all(orc, recs, 0, NAN_CLEAN)
        assert (o0["status"] & ~O.ST_FLIGHT).sum() == 0, "the 30 ticks in front of the poison are not clean"
        poisoned = clean.copy()
        for i in NAN_Z:
            poisoned["com_pos"][i, 2] = np.nan
        for i in NAN_ZD:
            poisoned["com_vel"][i, 2] = np.nan
        outs, _, fin = rollout_all(orc, poisoned, NAN_CLEAN, NAN_TICKS)
        healthy, _, _ = rollout_all(orc, clean, NAN_CLEAN, NAN_TICKS)
        pushed = clean.copy()
        for i in NAN_Z + NAN_ZD:
            pushed["com_vel"][i, 2] = pushed["com_vel"][i, 2] + np.nan
        mc_tail, _, mc_fin = rollout_all(orc, pushed, NAN_CLEAN, NAN_TICKS)
        mc_outs = np.concatenate([o0, mc_tail])
        frozen(recs, clean, poisoned, outs, fin, healthy, mc_outs, mc_fin)
        return dict(recs=recs, clean=clean, poisoned=poisoned, outs=outs, fin=fin, healthy_outs=healthy, mc_outs=mc_outs, mc_fin=mc_fin)
    return cached("nan100", make)


def nan_pushes(push_dtype):
    """The MC form's table: one entry per instance, dv[2] = NaN at tick 30 on the poisoned instances, padding (INT32_MAX) elsewhere."""
    p = np.zeros((B, 1), dtype=push_dtype)
    p["tick"] = 2 ** 31 - 1
    for i in NAN_Z + NAN_ZD:
        p["tick"][i, 0] = NAN_CLEAN
        p["dv"][i, 0, 2] = np.nan
    return p


# ---- zfail -----------------------------------------------------------------------------------------------------------------------------
def zfail_case():
    """N = 100, the default 40-row plan, z_ineq_lo = 1e-3: the oracle's verdict on the first tick (every instance Z_FAILED, none gated).
    Only that tick has a reference: the oracle feeds the failed tick back, the device by design does not."""
    def make():
        recs = initial_records()
        orc = O.Oracle(O.default_params(100, z_ineq_lo=ZFAIL_LO), backend="gi")
        ref = orc.solve(recs)[0]
        assert ((ref["status"] & O.ST_Z_FAILED) != 0).all() and ((ref["status"] & GATE_BITS) == 0).all(), ref["status"]
        frozen(recs, ref)
        return dict(recs=recs, first_tick=ref)
    return cached("zfail", make)


# ---- the caller's bookkeeping, restated (Controller.cpp:297-304 enabled, :310, :346-348, :503-504) --------------------------------------
def caller_loop(solve, recs, ftsp, control_dt, mpc_dt, first_frame, ticks):
    """The closed loop a caller drives himself around single ticks: `solve` maps tick_in records to tick_out records.  Returns (trajectory
    [ticks, B] as a list of record arrays, final state records)."""
    st = recs.copy()
    rows, traj = ftsp.shape[0], []
    for t in range(ticks):
        for i in range(len(st)):
            fc = int(st["footstep_counter"][i])
            if 0 <= fc < rows and st["simulation_time"][i] >= ftsp[fc, 3] - 1:                    # :297
                st["control_iter"][i] = 0; st["mpc_iter"][i] = 0; st["footstep_counter"][i] = fc + 1     # :298-300
        st["simulation_time"] = float(first_frame + t)                                            # :310
        out = solve(st)
        traj.append(out.copy())
        st["com_pos"] = out["com_pos"]; st["com_vel"] = out["com_vel"]                            # :346-348
        for i in range(len(st)):
            ctl = int(st["control_iter"][i]) + 1                                                  # :503
            st["control_iter"][i] = ctl
            st["mpc_iter"][i] = int(np.floor(ctl * control_dt / mpc_dt))                          # :504, (int)floor(ctl cdt / dt) as written
    return traj, st
