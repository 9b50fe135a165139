"""Test infrastructure: the predicted horizon of a Formulation A tick on the reference side -- the scripts' loop `compute prediction`
(walking/quad_walk_no_plots.m:297-314, trotting/quad_as_bip_no_plots.m:287-300) with up_to = C, plus the centre zc of every sample's ZMP
band from the adapted footsteps by exact_tick_a.mapping_weights (the integer rule of oracle/ismpc_oracle_a.c:560-569).

  predict_numpy   plain fp64 numpy
  predict_exact   the same loop in mpmath at exact_tick_a.DPS digits on fp64 inputs taken as exact, rounded once
  band_margin     w / 2 - |xz - zc| per sample: >= 0 inside the ZMP band, 0 on its edge

Both return [2 axes, 4, C]: x, xd, xz, zc at samples 1 .. C.  `dec` is [2, C + F]: u[0 .. C-1] then the absolute footsteps f[0 .. F-1].
Sample 1 is A_upd (x, xd + push, xz) + B_upd u[0], or -- with first=[2, 3] -- the given (x, xd, xz) per axis: the state a tick stored.
Sample i >= 2 is A_upd s + B_upd u[i-1].  mpmath is imported when predict_exact runs, not when this module is."""
import numpy as np

from helpers import exact_tick_a as X

ROWS = ("x", "xd", "xz", "zc")
AXIS_KEYS = (("x", "xd", "xz", "cur_x"), ("y", "yd", "yz", "cur_y"))


def _weights(par, state_before):
    rows = X.mapping_weights(par, int(state_before["fc"]), int(state_before["j"]))
    assert rows is not None, "mapping overflow: the tick leaves such an instance alone"
    return rows


def predict_numpy(par, state_before, push, dec, first=None):
    C, F, dt = par.C, par.F, par.dt
    dec = np.asarray(dec, dtype=np.float64)
    eta = np.sqrt(par.grav / par.height)
    ch, sh = np.cosh(eta * dt), np.sinh(eta * dt)
    Au = np.array([[ch, sh / eta, 1 - ch], [eta * sh, ch, -eta * sh], [0, 0, 1]]); Bu = np.array([dt - sh / eta, 1 - ch, dt])
    rows = _weights(par, state_before)
    pred = np.zeros((2, 4, C))
    for ax in (0, 1):
        kx, kv, kz, kc = AXIS_KEYS[ax]
        u, f = dec[ax, :C], dec[ax, C:C + F]
        if first is None:
            s = Au @ np.array([state_before[kx], np.float64(state_before[kv]) + np.float64(push[ax]), state_before[kz]]) + Bu * u[0]
        else:
            s = np.array(first[ax], dtype=np.float64)
        g = np.concatenate([[np.float64(state_before[kc])], f])
        for i in range(C):
            if i > 0:
                s = Au @ s + Bu * u[i]
            pf, rem = rows[i]
            pred[ax, :3, i] = s
            pred[ax, 3, i] = g[pf] if rem is None else (rem / par.ds) * g[pf] + (1.0 - rem / par.ds) * g[pf + 1]
    return pred


def predict_exact(par, state_before, push, dec, first=None):
    mp = X._mp()
    mpf = mp.mpf
    C, F = par.C, par.F
    dec = np.asarray(dec, dtype=np.float64)
    dt, eta = mpf(par.dt), mp.sqrt(mpf(par.grav) / mpf(par.height))
    ch, sh = mp.cosh(eta * dt), mp.sinh(eta * dt)
    A = ((ch, sh / eta, 1 - ch), (eta * sh, ch, -eta * sh), (mpf(0), mpf(0), mpf(1))); B = (dt - sh / eta, 1 - ch, dt)
    step = lambda s, u: [A[r][0] * s[0] + A[r][1] * s[1] + A[r][2] * s[2] + B[r] * u for r in range(3)]
    rows = _weights(par, state_before)
    pred = np.zeros((2, 4, C))
    for ax in (0, 1):
        kx, kv, kz, kc = AXIS_KEYS[ax]
        u = [mpf(float(v)) for v in dec[ax, :C]]
        g = [mpf(float(state_before[kc]))] + [mpf(float(v)) for v in dec[ax, C:C + F]]
        if first is None:
            vel = np.float64(state_before[kv]) + np.float64(push[ax])                      # formed once in fp64: data (exact_tick_a)
            s = step([mpf(float(state_before[kx])), mpf(float(vel)), mpf(float(state_before[kz]))], u[0])
        else:
            s = [mpf(float(v)) for v in first[ax]]
        for i in range(C):
            if i > 0:
                s = step(s, u[i])
            pf, rem = rows[i]
            zc = g[pf] if rem is None else (mpf(rem) / par.ds) * g[pf] + (1 - mpf(rem) / par.ds) * g[pf + 1]
            pred[ax, :, i] = [X._fp64(v) for v in s] + [X._fp64(zc)]
    return pred


def band_margin(par, pred):
    """w / 2 - |xz - zc|, [..., C]: the slack of ZMP row i against the nearer edge of its band."""
    pred = np.asarray(pred)
    return par.w / 2 - np.abs(pred[..., 2, :] - pred[..., 3, :])


def band_side(pred):
    """+1 where xz sits above the band's centre (the upper edge is the nearer one), -1 below: the sign convention of the fixtures' ws."""
    pred = np.asarray(pred)
    return np.where(pred[..., 2, :] >= pred[..., 3, :], 1, -1)


def first_of(state_after):
    """[2, 3]: (x, xd, xz) per axis of a STATE_A record -- what `first` takes."""
    return np.array([[state_after[k] for k in AXIS_KEYS[ax][:3]] for ax in (0, 1)], dtype=np.float64)
