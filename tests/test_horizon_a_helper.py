"""CPU-only: tests/helpers/horizon_a.py against the oracle it restates, and the floors file.

  * on the oracle's own whole solution of nominal and pushed walk and trot ticks, sample 1 of predict_numpy is the oracle's next state
    (1e-12, the tolerance tests/test_oracle_a.py holds restated arithmetic to) and predict_exact agrees with predict_numpy;
  * for every sample, lo_i <= dt cumsum(u)_i - (M f)_i <= hi_i of sim.axis_data holds if and only if |xz_i - zc_i| <= w / 2, outside the
    header's 1e-7 relative threshold around the edge -- which ties zc to the oracle's mapping;
  * tests/golden/formA_horizon_floors.npz loads, every entry finite and positive."""
import os

import numpy as np
import pytest

from helpers import exact_tick_a as X
from helpers import horizon_a as H

CASES = [("walk", 0, (0.0, 0.0)), ("walk", 37, (0.02, -0.03)), ("walk", 49, (0.0, 0.0)), ("walk", 75, (-0.015, 0.025)),
         ("trot", 0, (0.0, 0.0)), ("trot", 60, (0.018, -0.02)), ("trot", 79, (0.0, 0.0))]


@pytest.fixture(scope="module")
def A(built_libs):
    from oracle import oracle_a as A
    return A


@pytest.mark.parametrize("kind,ticks,push", CASES)
def test_prediction_restates_the_oracle(A, kind, ticks, push):
    k = A.WALK if kind == "walk" else A.TROT
    p = A.params(k)
    sim = A.SimA(A.gait(k, np.pi / 4, 0.1), p, backend="gi")
    for _ in range(ticks):
        sim.tick()
    par = X.Par(p)
    before = sim.state.copy()
    q = [sim.axis_data(ax) for ax in (0, 1)]
    r, sx, sy = sim.tick(push, want_solution=True)
    assert not r["rv"].any()
    after = sim.state.copy()
    dec = np.stack([sx, sy])
    pred = H.predict_numpy(par, before, push, dec)
    first = H.first_of(after)
    assert np.abs(pred[:, :3, 0] - first).max() <= 1e-12
    assert np.array_equal(H.predict_numpy(par, before, push, dec, first)[:, :3, 0], first)
    exact = H.predict_exact(par, before, push, dec)
    assert np.abs(exact - pred).max() <= 1e-9                       # the LIP's unstable mode over C samples; the floors file has the figures
    thr = 1e-7 * (1 + par.w / 2)
    m_pred = H.band_margin(par, pred)
    for ax in (0, 1):
        u, f = dec[ax, :par.C], dec[ax, par.C:]
        val = par.dt * np.cumsum(u) - q[ax]["M"][:, 1:] @ f
        m_orc = np.minimum(val - q[ax]["zlo"], q[ax]["zhi"] - val)
        clear = np.abs(m_orc) > thr
        assert np.array_equal(m_orc[clear] >= 0, m_pred[ax][clear] >= 0)
        assert np.abs(m_orc - m_pred[ax]).max() <= 1e-12
        assert (m_orc >= -thr).all()                                  # the oracle's solution is feasible


def test_floors_file():
    z = np.load(os.path.join(X.GOLDEN, "formA_horizon_floors.npz"))
    groups = ("walk_C100", "trot_C160", "edges", "inst_C200", "loop_walk_C100", "loop_trot_C65")
    assert sorted(z.files) == sorted(f"{g}_{k}" for g in groups for k in ("floor_u", "floor_f", "floor_pred"))
    for g in groups:
        assert z[f"{g}_floor_pred"].shape == (4,)
        for k in ("floor_u", "floor_f", "floor_pred"):
            v = np.asarray(z[f"{g}_{k}"])
            assert np.isfinite(v).all() and (v > 0).all(), (g, k, v)
    assert os.path.getsize(os.path.join(X.GOLDEN, "formA_horizon_floors.npz")) < 100_000
