"""CPU checks of the exact-arithmetic fixtures (tests/golden/formB_exact_<group>.npz, tests/helpers/exact_tick.py): the stored fp64
solutions satisfy the KKT conditions of both stages at rounding level in numpy.longdouble (no mpmath needed), mpmath regenerates them
byte for byte, the groups hold what tests/golden/make_golden_exact.py promises, and the shared comparison assert_exact accepts the fp64
oracle and rejects both the qpOASES goldens (1e-7-level termination error) and a 1e-9 relative perturbation."""
import os

import numpy as np
import pytest

from helpers import exact_tick as X

GROUPS = ("N100", "N100_zrows", "N37", "N50", "N128", "N129", "N200", "N100_stairs", "poly", "sweep4")
MIN_COUNT = {"N100": 40, "N100_zrows": 16, "N37": 12, "N50": 12, "N128": 12, "N129": 12, "N200": 12, "N100_stairs": 8, "poly": 12, "sweep4": 24}
LD = np.longdouble
U = LD(2.0) ** -53
SKIP = X.ST_TICK_SKIPPED | X.ST_BAD_INDEX
INFEASIBLE = X.ST_X_INFEASIBLE | X.ST_Y_INFEASIBLE


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    O.build()
    return O


def group_oracles(O, fx):
    sets = [O.Params.from_buffer_copy(bytes(b)) for b in fx["params"]]
    return sets, [O.Oracle(p, np.array(f), backend="gi") for p, f in zip(sets, fx["ftsp"])]


def oracle_records(O, fx):
    sets, orcs = group_oracles(O, fx)
    tin = fx["tick_in"].view(O.TICK_IN).reshape(-1)
    out = np.zeros(len(tin), dtype=O.TICK_OUT); traj = np.zeros((len(tin), 3, sets[0].N))
    for k, orc in enumerate(orcs):
        m = fx["set_idx"] == k
        out[m], _, traj[m] = orc.solve(tin[m], want_traj=True)
    return out, traj


# ---- the stored solutions are KKT points at rounding level (long double, no mpmath) ---------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_stored_solutions_satisfy_kkt_at_rounding_level(O, group):
    """Vertical stage: |H u + f + A'mu| <= 4 * 2^-53 (|H||u| + |f| + |A'||mu|) componentwise, the equality samples exactly zero, every row
    z_lo <= S u <= z_hi feasible to the rounding of u (2^-53 (|S_k||u| + |bound|)), multipliers of the right sign.  Horizontal stage:
    |a'u - beq| <= 4 * 2^-53 |a|'|u| with a, beq rebuilt in long double from the stored vertical trajectory, u inside the box mid +- half
    to one ulp.  H, f, a and beq are formed here in long double from the parameter bytes and the midpoint table."""
    fx = X.load_group(group)
    sets, orcs = group_oracles(O, fx)
    tin = fx["tick_in"].view(O.TICK_IN).reshape(-1)
    ref = fx["tick_out"].view(O.TICK_OUT).reshape(-1)
    n_v = n_h = 0
    for k, (p, orc) in enumerate(zip(sets, orcs)):
        N = p.N
        mid = orc.midpoint().astype(LD)
        dt, m, g = LD(p.mpc_dt), LD(p.mass), LD(p.g)
        c2 = dt * dt / m
        kk = np.arange(N)
        Si = np.where(kk[:, None] > kk[None, :], kk[:, None] - kk[None, :], 0).astype(np.int64)        # S = c2 Si, Sv = (dt/m) Vi
        Vi = (kk[:, None] > kk[None, :]).astype(np.int64)
        H = LD(p.q_p) * c2 * c2 * (Si.T @ Si).astype(LD) + LD(p.q_v) * (dt / m) ** 2 * (Vi.T @ Vi).astype(LD) + LD(p.q_u) * np.eye(N, dtype=LD)
        S = c2 * Si.astype(LD)
        eta = np.sqrt(g / LD(p.h_des))
        for b in np.flatnonzero(fx["set_idx"] == k):
            if ref["status"][b] & SKIP:
                continue
            idx = int(tin["simulation_time"][b] / (p.mpc_dt / p.control_dt))
            pos, vel = tin["com_pos"][b].astype(LD), tin["com_vel"][b].astype(LD)
            u = fx["u_traj"][b, 0].astype(LD)
            rp = pos[2] + (kk + 1) * dt * vel[2] - g * dt * dt * (kk * (kk + 1) // 2) - LD(p.h_des) - mid[idx:idx + N, 2]
            rv = vel[2] - g * dt * kk
            f = LD(p.q_p) * (S.T @ rp) + LD(p.q_v) * (dt / m) * (Vi.T.astype(LD) @ rv) - LD(p.q_u) * m * g
            mu_eq, mu_in = fx["mu_eq"][b].astype(LD), fx["mu_in"][b].astype(LD)
            r = H @ u + f + mu_eq + S.T @ mu_in
            bound = 4 * U * (np.abs(H) @ np.abs(u) + np.abs(f) + np.abs(mu_eq) + np.abs(S).T @ np.abs(mu_in))
            assert (np.abs(r) <= bound).all(), (group, b, float((np.abs(r) / bound).max()))
            assert (u[fx["eq_mask"][b]] == 0).all() and (mu_eq[~fx["eq_mask"][b]] == 0).all()
            sv, slack = S @ u, U * (np.abs(S) @ np.abs(u))
            assert (sv >= LD(p.z_ineq_lo) - slack - U * abs(p.z_ineq_lo)).all() and (sv <= LD(p.z_ineq_hi) + slack + U * abs(p.z_ineq_hi)).all(), (group, b)
            ws = fx["w_sign"][b]
            assert (mu_in[ws == 0] == 0).all() and (mu_in[ws != 0] * ws[ws != 0] > 0).all()
            act_bound = np.where(ws > 0, LD(p.z_ineq_hi), LD(p.z_ineq_lo))
            assert (np.abs(sv - act_bound)[ws != 0] <= (slack + U * np.abs(act_bound))[ws != 0]).all(), (group, b)
            assert bool(ref["status"][b] & X.ST_Z_INEQ_ACTIVE) == bool((ws != 0).any())
            n_v += 1
            # stage 2 and 3
            zpos = sv + pos[2] + (kk + 1) * dt * vel[2] - g * dt * dt * (kk * (kk + 1) // 2)
            lam = (u / m) / zpos
            assert abs(lam[0] - LD(fx["lambda0"][b])) <= 4 * U * abs(lam[0])
            assert bool(ref["status"][b] & X.ST_FLIGHT) == bool(not lam[0] > p.lambda_gate)
            if ref["status"][b] & X.ST_FLIGHT:
                assert (fx["u_traj"][b, 1:] == 0).all()
                continue
            half = LD(p.foot_width) / 2 if tin["footstep_counter"][b] > 1 else LD(p.first_step_halfwidth)
            r0, r1 = LD(1), 1 / eta
            a = np.zeros(N, dtype=LD)
            for i in range(N - 1, -1, -1):
                if lam[i] < p.lambda_gate:
                    A, B = (LD(1), dt, LD(0), LD(1)), (LD(0), LD(0))
                else:
                    sq = np.sqrt(lam[i]); ch, sh = np.cosh(sq * dt), np.sinh(sq * dt)
                    A, B = (ch, sh / sq, sq * sh, ch), (1 - ch, -sq * sh)
                a[i] = r0 * B[0] + r1 * B[1]
                r0, r1 = r0 * A[0] + r1 * A[2], r0 * A[1] + r1 * A[3]
            w = eta * dt * np.exp(-dt * eta * kk.astype(LD))
            for ax in (0, 1):
                if ref["status"][b] & (X.ST_X_INFEASIBLE, X.ST_Y_INFEASIBLE)[ax]:
                    assert fx["margins"][b, 2 + ax] < 0
                    continue
                beq = -(r0 * pos[ax] + r1 * vel[ax]) + w @ mid[idx + N:idx + 2 * N, ax]
                ux = fx["u_traj"][b, 1 + ax].astype(LD)
                assert abs(a @ ux - beq) <= 4 * U * (np.abs(a) @ np.abs(ux)), (group, b, ax, float(abs(a @ ux - beq) / (U * (np.abs(a) @ np.abs(ux)))))
                assert (np.abs(ux - mid[idx:idx + N, ax]) <= half + np.spacing(np.abs(fx["u_traj"][b, 1 + ax]))).all(), (group, b, ax)
                # the KKT form: one multiplier nu, u = clip(mid + nu a): the unclamped samples all give the stored nu
                free = np.abs(ux - mid[idx:idx + N, ax]) < half * (1 - LD(1e-12))
                free &= a != 0
                assert (N - int(free.sum()) - int((a == 0).sum())) == fx["clamped"][b, ax], (group, b, ax)
                nu = (ux - mid[idx:idx + N, ax])[free] / a[free]
                assert (np.abs(nu - LD(fx["nu"][b, ax])) * np.abs(a[free]) <= 4 * U * (np.abs(ux[free]) + np.abs(mid[idx:idx + N, ax][free]))).all(), (group, b, ax)
                n_h += 1
    assert n_v >= MIN_COUNT[group] and n_h >= 4


# ---- mpmath regenerates the fixtures byte for byte --------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_regenerated_instances_match_the_fixture_bytes(O, group):
    pytest.importorskip("mpmath")
    fx = X.load_group(group)
    sets, orcs = group_oracles(O, fx)
    tin = fx["tick_in"].view(O.TICK_IN).reshape(-1)
    picks = sorted({0, len(tin) - 1} | ({int(np.flatnonzero(fx["set_idx"] == k)[0]) for k in range(len(sets))} if group != "sweep4" else set()))
    assert len(picks) >= 2
    for b in picks:
        k = int(fx["set_idx"][b])
        hint = orcs[k].solve(tin[b:b + 1], want_traj=True)[2][0, 0]
        t = X.exact_tick(sets[k], orcs[k].midpoint(), tin[b], hint)
        assert X.certified(t)
        for name, v in X.instance_arrays(t).items():
            assert np.asarray(v).tobytes() == np.asarray(fx[name][b]).tobytes(), (group, b, name)


@pytest.mark.parametrize("group", ["N100", "N50"])
def test_regenerated_rollout_ticks_match_the_fixture_bytes(O, group):
    """The first three ticks of the group's first closed loop, and the stored floor is the oracle's own rollout against the stored one."""
    pytest.importorskip("mpmath")
    fx = X.load_group(group)
    sets, orcs = group_oracles(O, fx)
    tin = fx["tick_in"].view(O.TICK_IN).reshape(-1)
    j, i, frame = 0, int(fx["roll_sel"][0]), int(fx["roll_frame"][0])
    ins, outs, ref, ok = X.exact_rollout(sets[0], orcs[0].midpoint(), orcs[0], tin[i:i + 1], frame, 3)
    assert ok
    assert ins.tobytes() == fx["roll_in"][j][:3].tobytes() and outs.tobytes() == fx["roll_out"][j][:3].tobytes()


@pytest.mark.parametrize("group", ["N100", "N50"])
def test_rollout_floor_is_the_oracles_own_error(O, group):
    fx = X.load_group(group)
    sets, orcs = group_oracles(O, fx)
    tin = fx["tick_in"].view(O.TICK_IN).reshape(-1)
    ticks = fx["roll_out"].shape[1]
    worst = np.zeros(3)
    for j, (i, frame) in enumerate(zip(fx["roll_sel"], fx["roll_frame"])):
        ref, rin, _, _ = orcs[0].rollout(tin[i:i + 1], int(frame), ticks)
        want_in = fx["roll_in"][j].view(O.TICK_IN).reshape(-1)
        for k in ("simulation_time", "mpc_iter", "control_iter", "footstep_counter"):
            assert np.array_equal(rin[k], want_in[k])
        assert len(np.unique(rin["footstep_counter"])) >= 2                    # across a footstep switch
        e = X.assert_exact_rollout(ref, group, j)
        worst = np.maximum(worst, [e[k] for k in X.ROLL_QUANTITIES])
    assert np.array_equal(worst, fx["roll_floor"])
    # teeth: a CoM off by 1e-9 relative is rejected
    bad = ref.copy(); bad["com_pos"] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        X.assert_exact_rollout(bad, group, len(fx["roll_sel"]) - 1)


def test_passthrough_records(O):
    """A gated tick and a record outside the midpoint window: the state unchanged and the oracle's status bits."""
    pytest.importorskip("mpmath")
    st = O.initial_state(); st["footstep_counter"] = 1
    recs = np.repeat(st, 3)
    recs["simulation_time"] = [1700.0, -5.0, 3.0]; recs["mpc_iter"] = [0, 0, -2]
    p = O.default_params(100)
    orc = O.Oracle(p, backend="gi")
    for rec, ref in zip(recs, orc.solve(recs)[0]):
        t = X.exact_tick(p, orc.midpoint(), rec)
        o, traj = X.to_fp64(t)
        assert t.status == ref["status"] == X.ST_BAD_INDEX and np.array_equal(o["com_pos"], rec["com_pos"]) and not traj.any()
    p5 = O.default_params(20, mpc_dt=0.05, S=7, F=2)
    orc5 = O.Oracle(p5, O.reference_plan(S=7, F=2, mpc_dt=0.05), backend="gi")
    r = np.repeat(st, 2); r["control_iter"] = [3, 5]
    ref5 = orc5.solve(r)[0]
    got = [X.exact_tick(p5, orc5.midpoint(), rec, None).status for rec in r]
    assert got[0] == ref5["status"][0] == X.ST_TICK_SKIPPED and got[1] == ref5["status"][1]


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def test_group_composition():
    biggest = os.path.getsize(os.path.join(X.GOLDEN, "formB_vectors_N200.npz"))
    for group in GROUPS:
        fx = X.load_group(group)
        st = fx["tick_out"].view(X.TICK_OUT).reshape(-1)["status"]
        assert len(st) >= MIN_COUNT[group] and len(st) <= 64, group
        assert os.path.getsize(os.path.join(X.GOLDEN, f"formB_exact_{group}.npz")) <= biggest, group
        m = fx["margins"]
        assert (m[:, 0] > 1e-9).all() and (m[:, 1] > 1e-9).all(), group                       # strict complementarity; every lambda_j off the gate
        assert (np.abs(m[:, 2:][np.isfinite(m[:, 2:])]) > 1e-9).all(), group                  # off the feasibility boundary
        assert ((m[:, 2:] < 0).any(axis=1) == ((st & INFEASIBLE) != 0)).all(), group
        assert (fx["floor"] > 0).all() and (fx["floor"] < 1e-7).all(), group
    fx = X.load_group("N100")
    tin = fx["tick_in"].view(X.TICK_IN).reshape(-1)
    st = fx["tick_out"].view(X.TICK_OUT).reshape(-1)["status"]
    S = 35
    running = tin["footstep_counter"] > 1
    assert (running & (tin["mpc_iter"] < S)).sum() >= 8 and (running & (tin["mpc_iter"] >= S)).sum() >= 4
    assert (~running).sum() >= 3 and not fx["eq_mask"][~running].any() and fx["eq_mask"][running].any(axis=1).all()
    assert (np.abs(fx["u_traj"][~running, 1] - 0.0).max() > 0.045)                            # the first-step half width (1 m) is in use
    fed = (st & (INFEASIBLE | X.ST_FLIGHT)) == 0
    assert ((st & X.ST_FLIGHT) != 0).sum() >= 3
    assert (fed & (fx["clamped"][:, 0] > 0)).sum() >= 8 and (fed & (fx["clamped"][:, 1] > 0)).sum() >= 8
    assert ((st & X.ST_X_INFEASIBLE) != 0).sum() >= 2 and ((st & X.ST_Y_INFEASIBLE) != 0).sum() >= 2
    assert len(fx["shared_golden"]) >= 8 and len(fx["roll_sel"]) == 2 and fx["roll_out"].shape[1] == 40
    fx = X.load_group("N100_zrows")
    assert ((fx["w_sign"] > 0).any(axis=1) & (fx["set_idx"] == 0)).sum() >= 8 and ((fx["w_sign"] < 0).any(axis=1) & (fx["set_idx"] == 1)).sum() >= 8
    assert ((fx["tick_out"].view(X.TICK_OUT).reshape(-1)["status"] & X.ST_Z_INEQ_ACTIVE) != 0).all()
    assert (X.load_group("N100_stairs")["ftsp"][0][:, 2] != 0).any()
    cls = X.load_group("poly")["cls"]
    assert all((cls == c).sum() >= 4 for c in (0, 1, 2))
    assert all((X.load_group("sweep4")["set_idx"] == k).sum() >= 6 for k in range(4))
    assert len(X.load_group("N50")["roll_sel"]) == 2


# ---- the comparison has teeth -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_assert_exact_accepts_the_fp64_oracle_and_rejects_a_1e9_perturbation(O, group):
    fx = X.load_group(group)
    out, traj = oracle_records(O, fx)
    e = X.assert_exact(out, traj, group)
    assert np.array_equal([e[k] for k in X.QUANTITIES], fx["floor"])                          # the stored floor IS this error
    bad = traj.copy(); bad[:, 0] *= 1 + 1e-9
    with pytest.raises(AssertionError):
        X.assert_exact(out, bad, group)
    flip = out.copy(); flip["status"][0] ^= X.ST_FLIGHT
    with pytest.raises(AssertionError):
        X.assert_exact(flip, traj, group)


def test_assert_exact_rejects_the_qpoases_goldens():
    """The instances formB_vectors_N100.npz shares with the N100 group: the committed reference-qpOASES records and trajectories, good to
    its termination bound (2.2e-7 homotopy length), are NOT good to 16 x the fp64 floor."""
    fx = X.load_group("N100")
    z = np.load(os.path.join(X.GOLDEN, "formB_vectors_N100.npz"))
    shared = fx["shared_golden"]
    assert z["tick_in"][shared].tobytes() == fx["tick_in"][:len(shared)].tobytes()            # the same instances, first in the group
    out = np.ascontiguousarray(z["tick_out"][shared]).view(X.TICK_OUT).reshape(-1)
    traj = z["u_traj"][shared]
    assert np.array_equal(out["status"], fx["tick_out"].view(X.TICK_OUT).reshape(-1)["status"][:len(shared)])
    with pytest.raises(AssertionError):
        X.assert_exact(out, traj, "N100", sel=np.arange(len(shared)))
