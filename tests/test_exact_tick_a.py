"""CPU checks of the Formulation A exact-arithmetic fixtures (tests/golden/formA_exact_<group>.npz, tests/helpers/exact_tick_a.py): the
stored fp64 solutions are KKT points of the stored working sets at rounding level in numpy.longdouble (no mpmath needed), mpmath
regenerates the two small groups byte for byte, at least 90 % of the drawn ticks of every group were kept, the groups reach every kernel
instantiation, and the shared comparison assert_exact_a accepts the fp64 oracle at factor 1 and rejects both the reference's qpOASES
(run as a closed loop it stops about 2e-5 m/s short of the minimiser in u0) and a 1e-9 relative perturbation of the exact values."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import exact_tick_a as X

GROUPS = ("walk_C100", "trot_C160", "edges", "inst_C200", "loop_walk_C100", "loop_trot_C65")
SINGLE = GROUPS[:4]
LOOPS = GROUPS[4:]
COUNT = {"walk_C100": 16, "trot_C160": 16, "edges": 33, "inst_C200": 16, "loop_walk_C100": 62, "loop_trot_C65": 92}
LD = np.longdouble
U = LD(2.0) ** -53


@pytest.fixture(scope="module")
def M():
    """tests/golden/make_golden_exact_a.py as a module (the oracle side of the fixtures: states, hints, the floor's two evaluations)."""
    from oracle import oracle as O
    O.build()
    spec = importlib.util.spec_from_file_location("make_golden_exact_a", os.path.join(X.GOLDEN, "make_golden_exact_a.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    m.CENTERS = m.centers()
    return m


def rows_per_lane(C):
    return max(2, -(-C // 64))


def tick_inputs(fx, i):
    """(handle Par, plan index, center, STATE_A record, push, INST_A record or None) of tick i of a fixture."""
    par = X.Par(fx["params"][fx["case"][i]])
    inst = fx["inst"][i].view(X.INST_A)[0] if fx["has_inst"] else None
    return par, int(fx["plan"][i]), fx["centers"][fx["plan"][i]], fx["state"][i].view(X.STATE_A)[0], fx["push"][i], inst


# ---- composition ------------------------------------------------------------------------------------------------------------------------
def test_groups_cover_every_instantiation():
    """ismpc_a_tick_wave<Real, RL, F, PI>: RL = 2, 3, 4 and F = 3 .. 6 through the plain kernel, the per-instance kernel at the handle's
    F = 6 with F_i = 2 .. 6 (one launch per footstep count under ISMPC_A_BUCKET=1), both precisions through the handle's `precision`, and
    the workgroup kernel through ISMPC_A_KERNEL=block on the same groups (tests/test_gpu_exact_parity_a.py)."""
    plain, pi_f = set(), set()
    for g in SINGLE:
        fx = X.load_group(g)
        for i in range(len(fx["case"])):
            par, _, _, st, _, inst = tick_inputs(fx, i)
            if inst is None:
                plain.add((rows_per_lane(par.C), par.F))
            else:
                assert (rows_per_lane(par.C), par.F) == (4, 6)
                pi_f.add(int(inst["F"]))
    assert {rl for rl, _ in plain} == {2, 3, 4} and {F for _, F in plain} == {3, 4, 5, 6}
    assert plain == {(2, 3), (3, 3), (2, 4), (3, 5), (4, 6), (4, 3)}
    assert pi_f == {2, 3, 4, 5, 6}
    fx = X.load_group("edges")
    shapes = {(int(p[0]), int(p[2])) for p in fx["params"]}
    assert shapes == {(5, 3), (65, 4), (129, 5), (193, 6), (250, 6), (253, 3)}
    assert max(C + F for C, F in shapes) == 256                                  # the largest the handle takes
    for g in ("walk_C100", "trot_C160"):                                       # both centreline structures, both sides of a switch
        st = X.load_group(g)["state"].view(X.STATE_A).reshape(-1)
        after = X.load_group(g)["state_after"].view(X.STATE_A).reshape(-1)
        assert (st["rebuilt"] == 0).sum() >= 4 and (st["rebuilt"] == 1).sum() >= 4 and (after["fc"] != st["fc"]).sum() >= 2
    fx = X.load_group("inst_C200")                                               # per-instance: the bookkeeping of a switch in both plans,
    st, after = fx["state"].view(X.STATE_A).reshape(-1), fx["state_after"].view(X.STATE_A).reshape(-1)      # from either centreline structure
    inst = fx["inst"].view(X.INST_A).reshape(-1)
    sw = after["fc"] != st["fc"]
    assert (st["j"][sw] == inst["step"][sw] * st["fc"][sw] - 1).all() and (after["rebuilt"][sw] == 1).all()
    for plan in (0, 1):
        assert (sw & (inst["plan"] == plan) & (st["rebuilt"] == 0)).sum() >= 1 and (sw & (inst["plan"] == plan) & (st["rebuilt"] == 1)).sum() >= 1
    assert sw.sum() >= 6 and (~sw).sum() >= 6
    moved = (after["cur_x"] != st["cur_x"]) | (after["cur_y"] != st["cur_y"])      # (walk, Qf = 1e9: f0 can be the plan's footstep to the bit)
    shifted = (after["off_x"] != st["off_x"]) | (after["off_y"] != st["off_y"])
    assert not moved[~sw].any() and not shifted[~sw].any() and moved[sw].sum() >= 6 and shifted[sw].sum() >= 4
    assert (shifted & sw & (inst["plan"] == 0)).any() and (shifted & sw & (inst["plan"] == 1)).any()
    for g in LOOPS:
        fx = X.load_group(g)
        st, after = fx["state"].view(X.STATE_A).reshape(-1), fx["state_after"].view(X.STATE_A).reshape(-1)
        assert fx["loop"] == 1 and st[1:].tobytes() == after[:-1].tobytes() and (after["fc"] != st["fc"]).sum() == 1
        assert (np.abs(fx["push"]).max(1) > 0).sum() == (2 if g == "loop_walk_C100" else 1)


@pytest.mark.parametrize("group", GROUPS)
def test_kept_share_margins_and_size(group):
    fx = X.load_group(group)
    n = len(fx["case"])
    assert n == int(fx["kept"]) == COUNT[group] and fx["kept"] >= 0.9 * fx["drawn"]
    assert (fx["margins"][:, :, 0] >= X.MARGIN_SLACK).all() and (fx["margins"][:, :, 1] >= X.MARGIN_MULT).all()
    assert os.path.getsize(os.path.join(X.GOLDEN, f"formA_exact_{group}.npz")) <= 100_000
    assert np.array_equal(fx["floor"], np.maximum(fx["floor_oracle"], fx["floor_numpy"])) and "floor_round" not in fx
    assert (fx["floor"] > 0).all() and (fx["floor"] < 1e-9).all()
    act = X.active_sizes(fx["out"].view(X.OUT_A).reshape(-1))
    assert np.array_equal(act, 1 + (fx["ws"] != 0).sum(2))                       # the kernels' counting convention: the stability row counts


# ---- the stored solutions are KKT points at rounding level (long double, no mpmath) ---------------------------------------------------
def ld_problem(par, center, st, push, axis):
    """The axis' QP data in long double from the fixture's bytes: oracle/ismpc_oracle_a.c:197-223, 286-344 restated once more."""
    C, P, F, step, ds = par.C, par.P, par.F, par.step, par.ds
    j, fc = int(st["j"]), int(st["fc"])
    dt, eta = LD(par.dt), np.sqrt(LD(par.grav) / LD(par.height))
    pos, zmp = LD(st["xy"[axis]]), LD(st[("xz", "yz")[axis]])
    vel = LD(np.float64(st[("xd", "yd")[axis]]) + np.float64(push[axis]))
    cur, off = LD(st[("cur_x", "cur_y")[axis]]), LD(st[("off_x", "off_y")[axis]])
    fs = np.concatenate([[LD(0)], center[:, axis].astype(LD) + off])

    def cl(idx):
        blk, r = (idx - 1) // step, (idx - 1) % step
        if (blk == 0 and st["rebuilt"]) or r < step - ds:
            return fs[1] if blk == 0 else fs[blk + 1]
        k = r - (step - ds)
        return fs[blk + 1] if k == 0 else fs[blk + 2] if k == ds - 1 else fs[blk + 1] + (k * (fs[blk + 2] - fs[blk + 1])) / (ds - 1)
    lam = np.exp(-eta * dt)
    ii = np.arange(C + 1, P + 1)
    tail = np.array([cl(j + i) - cur for i in ii], dtype=LD)
    wts = np.exp(-eta * dt * ii.astype(LD)) * (1 - lam)
    anticip = wts @ tail + np.exp(-eta * dt * P) * (cl(P) - cur)
    a = (1 / eta) * (1 - lam) / (1 - lam ** C) * np.exp(-eta * dt * np.arange(C).astype(LD)) - dt * np.exp(-eta * dt * C)
    b = pos + vel / eta - zmp - anticip
    bmag = abs(pos) + abs(vel / eta) + abs(zmp) + np.abs(wts) @ np.abs(tail)
    Mz = np.zeros((C, F + 1), dtype=LD)
    for i, (pf, rem) in enumerate(X.mapping_weights(par, fc, j)):
        if rem is None:
            Mz[i, pf] = 1
        else:
            Mz[i, pf] = LD(rem) / ds; Mz[i, pf + 1] = 1 - LD(rem) / ds
    hi, lo = (-zmp + LD(par.w) / 2) + Mz[:, 0] * cur, (-zmp - LD(par.w) / 2) + Mz[:, 0] * cur
    d = np.full(F, LD(par.disp_forw) if axis == 0 else LD(par.disp_L))
    if fc == 1 and axis == 0:
        d[0] = LD(par.disp_forw_dummy)
    khi, klo = d.copy(), -d
    khi[0] += cur; klo[0] += cur
    return dict(a=a, b=b, bmag=bmag, M=Mz[:, 1:], lo=lo, hi=hi, klo=klo, khi=khi, pref=fs[fc + 1:fc + 1 + F], dt=dt, Qf=LD(par.Qf))


@pytest.mark.parametrize("group", GROUPS)
def test_stored_solutions_satisfy_kkt_at_rounding_level(group):
    """For the ticks whose whole solution is stored: |u + a mu_0 + dt suffix(mu)| and |Qf (f - p) - M'mu_z + D'mu_k| within 4 * 2^-53 of the
    sum of their terms' magnitudes, the stability row and every active row on its bound to the rounding of the stored point, every
    inactive row feasible, every multiplier of the sign of its bound; the first entries are the tick's u0 and f0."""
    fx = X.load_group(group)
    out = fx["out"].view(X.OUT_A).reshape(-1)
    n_checked = n_active = 0
    for k, i in enumerate(fx["sol_idx"]):
        par, _, center, st, push, inst = tick_inputs(fx, i)
        par = X.Par(par, inst)
        C, F = par.C, par.F
        for ax in (0, 1):
            q = ld_problem(par, center, st, push, ax)
            u, f = fx["sol"][k, ax, :C].astype(LD), fx["sol"][k, ax, C:C + F].astype(LD)
            mu = fx["mu"][k, ax].astype(LD)
            ws = fx["ws"][i, ax]
            assert not ws[C + F:].any() and (mu[1:][ws == 0] == 0).all()
            mz, mk = mu[1:C + 1], mu[C + 1:C + F + 1]
            suf = np.cumsum(mz[::-1])[::-1]
            r = u + q["a"] * mu[0] + q["dt"] * suf
            bound = 4 * U * (np.abs(u) + np.abs(q["a"] * mu[0]) + q["dt"] * np.cumsum(np.abs(mz)[::-1])[::-1])
            assert (np.abs(r) <= bound).all(), (group, i, ax, float((np.abs(r) / bound).max()))
            dk = mk - np.concatenate([mk[1:], [LD(0)]])                          # D' mu_k
            rf = q["Qf"] * (f - q["pref"]) - q["M"].T @ mz + dk
            bf = 4 * U * (q["Qf"] * (np.abs(f) + np.abs(q["pref"])) + np.abs(q["M"]).T @ np.abs(mz) + np.abs(mk) + np.abs(np.concatenate([mk[1:], [LD(0)]])))
            assert (np.abs(rf) <= bf).all(), (group, i, ax, float((np.abs(rf) / bf).max()))
            assert abs(q["a"] @ u - q["b"]) <= 4 * U * (np.abs(q["a"]) @ np.abs(u) + q["bmag"]), (group, i, ax)
            zv = q["dt"] * np.cumsum(u) - q["M"] @ f
            zs = U * (q["dt"] * np.cumsum(np.abs(u)) + np.abs(q["M"]) @ np.abs(f) + np.maximum(np.abs(q["lo"]), np.abs(q["hi"])))
            kv = f - np.concatenate([[LD(0)], f[:-1]])
            ks = U * (np.abs(f) + np.concatenate([[LD(0)], np.abs(f[:-1])]) + np.maximum(np.abs(q["klo"]), np.abs(q["khi"])))
            v, s = np.concatenate([zv, kv]), 4 * np.concatenate([zs, ks])
            lo, hi = np.concatenate([q["lo"], q["klo"]]), np.concatenate([q["hi"], q["khi"]])
            w = ws[:C + F]
            assert (v >= lo - s).all() and (v <= hi + s).all(), (group, i, ax)
            assert (np.abs(v - hi)[w > 0] <= s[w > 0]).all() and (np.abs(v - lo)[w < 0] <= s[w < 0]).all(), (group, i, ax)
            assert (mu[1:C + F + 1][w != 0] * w[w != 0] > 0).all(), (group, i, ax)
            slack = np.minimum(v - lo, hi - v)[w == 0]
            assert slack.min() >= LD(fx["margins"][i, ax, 0]) * (1 - LD(1e-6)) - s.max(), (group, i, ax)
            assert u[0] == out["u0"][i, ax] and f[0] == out["f0"][i, ax]
            n_checked += 1; n_active += int((w != 0).sum())
    assert n_checked >= 16 and n_active >= 100


# ---- mpmath regenerates the two small groups byte for byte ------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["edges", "inst_C200"])
def test_regenerated_group_matches_the_fixture_bytes(M, group):
    pytest.importorskip("mpmath")
    fx = X.load_group(group)
    g, _ = M.build_group(group)
    n = len(g)
    assert n == len(fx["case"]) and g.drawn == fx["drawn"]
    width = fx["ws"].shape[2]
    rows = [X.tick_arrays(t, width) for t in g.ticks]
    assert np.array(g.state).tobytes() == fx["state"].tobytes() and np.stack(g.push).tobytes() == fx["push"].tobytes()
    assert np.array(g.inst).tobytes() == fx["inst"].tobytes() and np.stack([p.row() for p in g.pars]).tobytes() == fx["params"].tobytes()
    assert np.array(g.outs).tobytes() == fx["out"].tobytes() and np.array(g.afters).tobytes() == fx["state_after"].tobytes()
    assert np.stack([r["ws"] for r in rows]).tobytes() == fx["ws"].tobytes()
    assert np.stack([r["margins"] for r in rows]).tobytes() == fx["margins"].tobytes()
    assert np.stack([rows[i]["sol"] for i in fx["sol_idx"]]).tobytes() == fx["sol"].tobytes()
    assert np.stack([rows[i]["mu"] for i in fx["sol_idx"]]).tobytes() == fx["mu"].tobytes()
    for t in g.ticks:                                                          # the certificate each of them passed
        assert all(r["residual"] <= X.CERT_REL and r["stationarity"] <= X.CERT_REL and not r["violated"] for r in t.axes)


# ---- the comparison has teeth -----------------------------------------------------------------------------------------------------------
def oracle_quantities(M, fx, backend="gi"):
    """The fp64 oracle on the fixture's own inputs: single ticks through load_product_state, a loop as the oracle's own loop."""
    n = len(fx["case"])
    if fx["loop"]:
        par, kind, _, _, _, _ = tick_inputs(fx, 0)
        pushes = {t: tuple(fx["push"][t]) for t in range(n) if np.abs(fx["push"][t]).max() > 0}
        states, recs = M.nominal_states(kind, par, n, pushes, backend)
        o = np.zeros(n, X.OUT_A)
        for k in ("com_before", "vel_after", "u0", "f0"):
            o[k] = np.array([r[k] for r in recs])
        return X.quantities(o, np.array(states[1:]))
    outs, afters = [], []
    for i in range(n):
        par, kind, center, st, push, inst = tick_inputs(fx, i)
        sim = M.make_sim(kind, X.Par(par, inst), backend)
        o, s, _, rv = M.oracle_tick(sim, center, st, push)
        assert not rv.any()
        outs.append(o); afters.append(s)
    return X.quantities(np.array(outs), np.array(afters))


@pytest.mark.parametrize("group", GROUPS)
def test_assert_exact_a_accepts_the_fp64_oracle_and_rejects_a_1e9_perturbation(M, group):
    fx = X.load_group(group)
    exact, floor = X.fixture_exact(fx), X.group_floor(fx)
    got = oracle_quantities(M, fx)
    e = X.assert_exact_a(got, exact, floor, factor=1, same_input=not fx["loop"])
    e = X.reference_floor(e)                                                     # (cur / off: at least the f0 error)
    assert np.array_equal([e[k] for k in X.QUANTITIES], fx["floor_oracle"])      # the stored oracle floor IS this error
    bad = {k: (v * (1 + 1e-9) if k in X.QUANTITIES else v) for k, v in exact.items()}      # the exact values, off by 1e-9 relative
    with pytest.raises(AssertionError):
        X.assert_exact_a(bad, exact, floor)
    for k in ("com",):                                                           # ... and one quantity alone
        bad = dict(exact); bad[k] = exact[k] * (1 + 1e-9)
        with pytest.raises(AssertionError):
            X.assert_exact_a(bad, exact, floor)
    for k in X.COUNTERS:
        flip = dict(exact); flip[k] = exact[k].copy(); flip[k][0] ^= 1
        with pytest.raises(AssertionError):
            X.assert_exact_a(flip, exact, floor)
    X.assert_exact_a(exact, exact, floor, factor=0)


@pytest.mark.parametrize("group", LOOPS)
def test_assert_exact_a_rejects_the_reference_qp_solver(M, group):
    """qpOASES as the reference configures it, run as the oracle's own closed loop with the fixture's pushes: good to its own termination
    bound (TOL_U0["ref"] = 6e-5 of tests/test_gpu_formulation_a.py), NOT good to 16 x the fp64 floor.  (Started cold on a single tick it
    lands within 1e-9 m/s of the minimiser; in a closed loop every tick starts from the previous one's homotopy and stops short.)"""
    from oracle import oracle as O
    if not O.have_ref():
        pytest.skip("oracle/_ref (the reference's qpOASES) is not built here")
    fx = X.load_group(group)
    exact, floor = X.fixture_exact(fx), X.group_floor(fx)
    got = oracle_quantities(M, fx, backend="ref")
    err = np.abs(got["u0"] - exact["u0"]).max()
    print("qpOASES u0 error", err, "floor", floor["u0"])
    assert err <= 6e-5
    with pytest.raises(AssertionError):
        X.assert_exact_a(got, exact, floor, same_input=False)
    counters_only = dict(exact); counters_only.update({k: got[k] for k in X.COUNTERS})
    X.assert_exact_a(counters_only, exact, floor, same_input=False)               # ... and it is the values that are rejected, not a counter


@pytest.mark.parametrize("group", SINGLE)
def test_reference_qp_solver_on_cold_single_ticks(M, group):
    """The same solver started cold on the single-tick groups: it ends within 1e-9 m/s of the minimiser there, which is inside or at
    16 x the floor of every one of them (u0 error over the bound: walk_C100 0.63, trot_C160 1.06, edges 0.03, inst_C200 0.09 -- the floors
    are set by a plain KKT solve that is no better conditioned).  So the single-tick groups would NOT reliably reject it; the figures are
    printed, only the size of the error is asserted, and the control with teeth is the closed loop above."""
    from oracle import oracle as O
    if not O.have_ref():
        pytest.skip("oracle/_ref (the reference's qpOASES) is not built here")
    fx = X.load_group(group)
    exact, floor = X.fixture_exact(fx), X.group_floor(fx)
    got = oracle_quantities(M, fx, backend="ref")
    e = X.errors(got, exact)
    print("qpOASES cold", group, {k: (e[k], e[k] / (X.BOUND_FACTOR * floor[k])) for k in X.QUANTITIES})
    assert e["u0"] <= 1e-8 and all(np.array_equal(got[k], exact[k]) for k in X.COUNTERS)
