"""Test infrastructure: one Formulation A tick (oracle/ismpc_oracle_a.c:197-223 centreline, 286-344 the per-axis QP, 548-615 the tick) in
exact arithmetic -- mpmath at DPS digits -- plus the comparison the rounding-level tests share (assert_exact_a).

The problem data are fp64 numbers taken as exact: the ismpc_a_params fields, an ismpc_a_inst record where one is given (it overrides
height, Qf, step, ds, F), the ismpc_a_state record (off_x, off_y, rebuilt included), the base plan `center` as FA.plan returns it, and the
tick's pushed velocity xd + push, formed ONCE in fp64 as include/ismpc_a.h states.  Everything derived -- eta, lambda, the stability row,
the centreline rebuilt from center + off by the linspace rule (initial or rebuilt structure), the anticipative tail, rem / ds, the ZMP
band, the kinematic bounds, b, cosh / sinh of the LIP update, the footstep bookkeeping -- is evaluated in mpmath and rounded once, at
the end.

The per-axis QP   min 1/2 |u|^2 + Qf/2 |f - p|^2   s.t.  a'u = b,  lo <= dt cumsum(u) - M f <= hi  (C rows),  klo <= D f <= khi  (F rows)
is strictly convex with a diagonal Hessian.  This file is not a QP solver: it takes a HINT (the rows of the fp64 oracle's solution
within HINT_BAND of a bound), solves the equality-constrained problem of that working set and CERTIFIES the point in mpmath:
active-row residuals and stationarity <= CERT_REL (the point is formed from the multipliers by the stationarity equations, so that part
holds by construction; both are evaluated on the final point), every inactive row feasible, every multiplier of the right sign.  Strict
convexity plus the certificate makes the point the unique minimiser, whatever route found it.  The solve is iterative refinement on the
multipliers: the Schur complement A_W H^-1 A_W' (order |W| + 1) is factorised in fp64 as the preconditioner, the primal point is formed
from the multipliers and the residuals of the active rows are evaluated in mpmath; every pass gains the digits the fp64 solve has.  The
smallest slack of an inactive row and the smallest multiplier relative to the largest are the tick's margins.  (If the hinted set does not
certify, rows with a wrong-sign multiplier leave and violated rows enter, at most REPAIR_ROUNDS times: the certificate decides, not the
route.)  QPs without a feasible point and ticks with a mapping overflow or an index outside the plan are out of scope: ExactTickA.ok is
False there.

mpmath is imported when a tick is computed, not when this module is: assert_exact_a and the fixture loader run without it.
"""
import os

import numpy as np

DPS = 50
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
BOUND_FACTOR = 16          # four bits over a plain fp64 evaluation (the stored floor): summation order, table precision
F32_RATIO = 2.0 ** 29      # unit roundoff of fp32 over that of fp64: the fp32 floor is the stored fp64 floor times this
HINT_BAND = 1e-9           # rows of the hint within this distance of a bound form the candidate working set
CERT_REL = 1e-40
REPAIR_ROUNDS = 3
MARGIN_SLACK, MARGIN_MULT = 1e-8, 1e-6          # a tick enters a fixture when both QPs certify with at least these margins
QUANTITIES = ("u0", "f0", "com", "vel", "zmp", "cur_off")
COUNTERS = ("status", "fc", "j", "rebuilt")
PARAM_FIELDS = ("C", "P", "F", "step", "ds", "n_gait", "dt", "height", "grav", "w", "Qf", "disp_forw", "disp_forw_dummy", "disp_L")
INT_FIELDS = PARAM_FIELDS[:6]

STATE_A = np.dtype([("x", "<f8"), ("xd", "<f8"), ("xz", "<f8"), ("y", "<f8"), ("yd", "<f8"), ("yz", "<f8"),
                    ("cur_x", "<f8"), ("cur_y", "<f8"), ("off_x", "<f8"), ("off_y", "<f8"),
                    ("fc", "<i4"), ("j", "<i4"), ("rebuilt", "<i4"), ("reserved", "<i4")], align=False)
OUT_A = np.dtype([("com_before", "<f8", 2), ("vel_after", "<f8", 2), ("u0", "<f8", 2), ("f0", "<f8", 2),
                  ("status", "<i4"), ("iters_x", "<i4"), ("iters_y", "<i4"), ("active", "<i4")], align=False)
INST_A = np.dtype([("height", "<f8"), ("Qf", "<f8"), ("step", "<i4"), ("ds", "<i4"), ("F", "<i4"), ("plan", "<i4")], align=False)


class Par:
    """The ismpc_a_params fields as plain attributes (from a ctypes structure, a fixture row or another Par), an inst record applied."""

    def __init__(self, src, inst=None):
        for k in PARAM_FIELDS:
            v = src[PARAM_FIELDS.index(k)] if isinstance(src, (np.ndarray, list, tuple)) else getattr(src, k)
            setattr(self, k, int(v) if k in INT_FIELDS else float(v))
        if inst is not None:
            self.height, self.Qf = float(inst["height"]), float(inst["Qf"])
            self.step, self.ds, self.F = int(inst["step"]), int(inst["ds"]), int(inst["F"])

    def row(self):
        return np.array([float(getattr(self, k)) for k in PARAM_FIELDS])


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


class ExactTickA:
    """Everything one exact tick produced (mpf values); to_records rounds once."""
    pass


def mapping_weights(p, fc, j):
    """[(first mapped footstep pf, rem or None)] per row i = 1 .. C as oracle/ismpc_oracle_a.c:560-569 -- rem None: weight 1 on column pf,
    else rem / ds on pf and 1 - rem / ds on pf + 1 -- or None on overflow (integers: decided as the oracle decides it)."""
    rows, pf = [], 0
    for i in range(1, p.C + 1):
        if j + i >= p.step * (fc + pf):
            pf += 1
        rem = p.step * (fc + pf) - (j + i)
        if pf + 1 > p.F + 1 or (rem <= p.ds and pf + 2 > p.F + 1):
            return None
        rows.append((pf, None if rem > p.ds else rem))
    return rows


def _centreline(mp, p, fs, rebuilt):
    """cl(idx), 1-based, of oracle/ismpc_oracle_a.c:200-223 over fs (1-based list of mpf): MATLAB linspace inside each double-support."""
    step, ds = p.step, p.ds

    def cl(idx):
        blk, r = (idx - 1) // step, (idx - 1) % step
        i = blk + 1                                                   # fs index of the block's stance footstep
        assert 1 <= i <= p.n_gait - 1, idx
        if blk == 0 and rebuilt:
            return fs[1]
        if r < step - ds:
            return fs[i]
        k = r - (step - ds)
        if k == 0:
            return fs[i]
        if k == ds - 1:
            return fs[i + 1]
        return fs[i] + (k * (fs[i + 1] - fs[i])) / (ds - 1)
    return cl


def _axis_problem(mp, p, center, st, vel, axis, rows):
    """The data of one axis' QP in mpf: a [C], b, lo / hi [C], klo / khi [F], pref [F], Qf, dt."""
    mpf = mp.mpf
    C, P, F = p.C, p.P, p.F
    j, fc = int(st["j"]), int(st["fc"])
    dt, eta = mpf(p.dt), mp.sqrt(mpf(p.grav) / mpf(p.height))
    pos, zmp = mpf(float(st["xy"[axis]])), mpf(float(st[("xz", "yz")[axis]]))
    cur, off = mpf(float(st[("cur_x", "cur_y")[axis]])), mpf(float(st[("off_x", "off_y")[axis]]))
    fs = [None] + [mpf(float(center[i, axis])) + off for i in range(p.n_gait)]
    cl = _centreline(mp, p, fs, int(st["rebuilt"]) != 0)
    lam = mp.exp(-eta * dt)
    anticip = mp.fsum(mp.exp(-eta * dt * i) * (1 - lam) * (cl(j + i) - cur) for i in range(C + 1, P + 1))
    anticip += mp.exp(-eta * dt * P) * (cl(P) - cur)
    a = [(1 / eta) * (1 - lam) / (1 - lam ** C) * mp.exp(-eta * dt * i) - dt * mp.exp(-eta * dt * C) for i in range(C)]
    b = pos + mpf(float(vel)) / eta - zmp - anticip
    w = mpf(p.w)
    m1 = [(mpf(1) if rem is None else mpf(rem) / p.ds) if pf == 0 else mpf(0) for pf, rem in rows]
    hi = [(-zmp + w / 2) + m * cur for m in m1]
    lo = [(-zmp - w / 2) + m * cur for m in m1]
    klo, khi = [], []
    for r in range(1, F + 1):
        d = mpf(p.disp_forw) if axis == 0 else mpf(p.disp_L) / 2 + mpf(p.disp_L) / 2
        if fc == 1 and r == 1 and axis == 0:
            d = mpf(p.disp_forw_dummy)
        khi.append(d + cur if r == 1 else d)
        klo.append(-(d - cur) if r == 1 else -d)
    pref = [fs[fc + 1 + k] for k in range(F)]
    return dict(a=a, b=b, lo=lo, hi=hi, klo=klo, khi=khi, pref=pref, Qf=mpf(p.Qf), dt=dt, eta=eta)


def _dense_rows(p, q, rows, W):
    """fp64: (A_W [1 + |W|, C + F], d_W, H^-1 diagonal) of the working set W = [(row, sign)], row 1 .. C ZMP, C + 1 .. C + F kinematic."""
    C, F = p.C, p.F
    A = np.zeros((1 + len(W), C + F)); d = np.zeros(1 + len(W))
    A[0, :C] = [float(v) for v in q["a"]]; d[0] = float(q["b"])
    for n, (i, s) in enumerate(W, 1):
        if i <= C:
            pf, rem = rows[i - 1]
            A[n, :i] = p.dt
            wgt = 1.0 if rem is None else rem / p.ds
            if pf >= 1:
                A[n, C + pf - 1] = -wgt
            if rem is not None:
                A[n, C + pf] = -(1.0 - wgt)
            d[n] = float(q["hi"][i - 1] if s > 0 else q["lo"][i - 1])
        else:
            r = i - C
            A[n, C + r - 1] = 1.0
            if r >= 2:
                A[n, C + r - 2] = -1.0
            d[n] = float(q["khi"][r - 1] if s > 0 else q["klo"][r - 1])
    hinv = np.concatenate([np.ones(C), np.full(F, 1.0 / p.Qf)])
    return A, d, hinv


def _primal(mp, p, q, rows, W, mu):
    """(u, f) = -H^-1 (g + A_W' mu) in mpf: u_k = -a_k mu_0 - dt sum of mu over the active ZMP rows i > k; f_r = p_r - (A_W' mu)_r / Qf."""
    mpf = mp.mpf
    C, F = p.C, p.F
    at = [mpf(0)] * (C + 2)                                            # multiplier of ZMP row i (0 where inactive)
    gf = [mpf(0)] * F                                                  # (A_W' mu) on the footstep columns
    for n, (i, s) in enumerate(W, 1):
        if i <= C:
            at[i] = mu[n]
            pf, rem = rows[i - 1]
            wgt = mpf(1) if rem is None else mpf(rem) / p.ds
            if pf >= 1:
                gf[pf - 1] -= wgt * mu[n]
            if rem is not None:
                gf[pf] -= (1 - wgt) * mu[n]
        else:
            r = i - C
            gf[r - 1] += mu[n]
            if r >= 2:
                gf[r - 2] -= mu[n]
    u, suf = [None] * C, mpf(0)
    for k in range(C - 1, -1, -1):
        suf += at[k + 1]
        u[k] = -q["a"][k] * mu[0] - q["dt"] * suf
    f = [q["pref"][r] - gf[r] / q["Qf"] for r in range(F)]
    return u, f


def _row_values(mp, p, q, rows, u, f):
    """(ZMP row values [C], kinematic row values [F], a'u) in mpf."""
    mpf = mp.mpf
    zv, cs = [], mpf(0)
    for i in range(1, p.C + 1):
        cs += u[i - 1]
        pf, rem = rows[i - 1]
        wgt = mpf(1) if rem is None else mpf(rem) / p.ds
        m = (wgt * f[pf - 1] if pf >= 1 else mpf(0)) + ((1 - wgt) * f[pf] if rem is not None else mpf(0))
        zv.append(q["dt"] * cs - m)
    kv = [f[r] - (f[r - 1] if r >= 1 else mpf(0)) for r in range(p.F)]
    return zv, kv, mp.fdot(q["a"], u)


def _solve_axis(mp, p, q, rows, hint):
    """The certified minimiser of one axis.  Returns a dict (u, f, mu, W, slack, mult, certified)."""
    mpf = mp.mpf
    C, F = p.C, p.F
    hz, hk, _ = _row_values(mp, p, q, rows, [mpf(float(v)) for v in hint[:C]], [mpf(float(v)) for v in hint[C:C + F]])
    W = []
    for i in range(1, C + 1):
        if abs(hz[i - 1] - q["hi"][i - 1]) <= HINT_BAND:
            W.append((i, 1))
        elif abs(hz[i - 1] - q["lo"][i - 1]) <= HINT_BAND:
            W.append((i, -1))
    for r in range(1, F + 1):
        if abs(hk[r - 1] - q["khi"][r - 1]) <= HINT_BAND:
            W.append((C + r, 1))
        elif abs(hk[r - 1] - q["klo"][r - 1]) <= HINT_BAND:
            W.append((C + r, -1))
    res = None
    for _ in range(REPAIR_ROUNDS + 1):
        res = _solve_working_set(mp, p, q, rows, W)
        if res["certified"] or not res["solved"]:
            break
        keep = [(i, s) for (i, s), m in zip(W, res["mu"][1:]) if s * m > 0]
        have = {i for i, _ in keep}
        W = sorted(keep + [(i, s) for i, s in res["violated"] if i not in have])
    return res


def _solve_working_set(mp, p, q, rows, W):
    mpf = mp.mpf
    C, F = p.C, p.F
    A, d, hinv = _dense_rows(p, q, rows, W)
    S = (A * hinv) @ A.T
    sc = 1.0 / np.sqrt(np.diag(S))
    Ss = S * sc[:, None] * sc[None, :]
    try:
        Sinv = np.linalg.inv(Ss)
    except np.linalg.LinAlgError:
        return dict(solved=False, certified=False, W=W)
    dW = [q["b"]] + [(q["hi"][i - 1] if s > 0 else q["lo"][i - 1]) if i <= C else (q["khi"][i - C - 1] if s > 0 else q["klo"][i - C - 1]) for i, s in W]
    scale = [max(abs(v), mpf(1e-3)) for v in dW]                     # residuals relative to the bound's size (positions of a step's size)
    mu = [mpf(0)] * (1 + len(W))
    solved = False
    for _ in range(40):
        u, f = _primal(mp, p, q, rows, W, mu)
        zv, kv, au = _row_values(mp, p, q, rows, u, f)
        r = [au - dW[0]] + [(zv[i - 1] if i <= C else kv[i - C - 1]) - dW[n] for n, (i, s) in enumerate(W, 1)]
        rel = max(abs(v) / sc_ for v, sc_ in zip(r, scale))
        if rel <= mpf(CERT_REL) / 10:
            solved = True
            break
        big = max(abs(v) for v in r)
        rn = np.array([float(v / big) for v in r])
        delta = sc * (Sinv @ (sc * rn))
        mu = [m + big * mpf(float(dl)) for m, dl in zip(mu, delta)]
    out = dict(solved=solved, certified=False, W=W, mu=mu)
    if not solved:
        return out
    # between two consecutive active rows on the same bound u is exactly zero; the solve leaves 1e-DPS there, whose digits depend on
    # the fp64 preconditioner.  A component below 1e-30 of the largest is that residue and is set to the zero it stands for
    big = max(abs(v) for v in u)
    u = [v if abs(v) > big * mpf(10) ** (20 - DPS) else mpf(0) for v in u]
    # ---- the certificate, evaluated on the FINAL point (after the zeroing above): the rows and the residual of the active ones again,
    # and stationarity over every variable.  u and f were formed from mu by the stationarity equations, so the latter holds by
    # construction up to the zeroed residues; it is evaluated here so that the certificate reads off the point that is stored, and
    # tests/test_exact_tick_a.py re-checks it independently in long double from the stored fp64 numbers.
    zv, kv, au = _row_values(mp, p, q, rows, u, f)
    r = [au - dW[0]] + [(zv[i - 1] if i <= C else kv[i - C - 1]) - dW[n] for n, (i, s) in enumerate(W, 1)]
    rel = max(abs(v) / sc_ for v, sc_ in zip(r, scale))
    at = {i: mu[n] for n, (i, s) in enumerate(W, 1)}
    stat, suf = mpf(0), mpf(0)
    for k in range(C - 1, -1, -1):                                     # d/du_k: u_k + a_k mu_0 + dt (sum of mu over ZMP rows i > k)
        suf += at.get(k + 1, mpf(0))
        stat = max(stat, abs(u[k] + q["a"][k] * mu[0] + q["dt"] * suf))
    for r_ in range(1, F + 1):                                         # d/df_r: Qf (f_r - p_r) - M' mu_z + D' mu_k, relative to Qf
        gz = mpf(0)
        for i in range(1, C + 1):
            if i in at:
                pf, rem = rows[i - 1]
                wgt = mpf(1) if rem is None else mpf(rem) / p.ds
                gz += (wgt if pf == r_ else mpf(0)) * at[i] + ((1 - wgt) if (rem is not None and pf + 1 == r_) else mpf(0)) * at[i]
        gk = at.get(C + r_, mpf(0)) - at.get(C + r_ + 1, mpf(0)) if r_ < F else at.get(C + r_, mpf(0))
        stat = max(stat, abs(q["Qf"] * (f[r_ - 1] - q["pref"][r_ - 1]) - gz + gk) / q["Qf"])
    active = dict(W)
    slack, violated = mp.inf, []
    for i in range(1, C + F + 1):
        v = zv[i - 1] if i <= C else kv[i - C - 1]
        lo = q["lo"][i - 1] if i <= C else q["klo"][i - C - 1]
        hi = q["hi"][i - 1] if i <= C else q["khi"][i - C - 1]
        if i in active:
            other = (v - lo) if active[i] > 0 else (hi - v)
            slack = min(slack, other)
        else:
            slack = min(slack, v - lo, hi - v)
            if v < lo:
                violated.append((i, -1))
            elif v > hi:
                violated.append((i, 1))
    mults = [s * m for (i, s), m in zip(W, mu[1:])]
    mult = (min(mults) / max(abs(m) for m in mults)) if mults else mp.inf
    out.update(u=u, f=f, slack=slack, mult=mult, violated=violated, residual=rel, stationarity=stat,
               certified=bool(rel <= CERT_REL and stat <= CERT_REL and slack >= 0 and mult > 0 and not violated))
    return out


def exact_tick_a(params, center, state, push=(0.0, 0.0), inst=None, hint=None):
    """One tick.  params: anything with the ismpc_a_params fields; center: the instance's base plan [n_gait, 2]; state: one STATE_A record;
    push: the tick's (px, py); inst: an INST_A record or None; hint: the fp64 oracle's (sol_x, sol_y), each C + F values."""
    mp = _mp()
    mpf = mp.mpf
    p = Par(params, inst)
    t = ExactTickA()
    t.p, t.ok, t.state_in = p, False, state
    j, fc = int(state["j"]), int(state["fc"])
    rows = mapping_weights(p, fc, j)
    if rows is None or fc + p.F > p.n_gait or j + p.P > p.step * (p.n_gait - 1) or not (p.step * (fc - 1) <= j <= p.step * fc - 1):
        return t
    t.rows = rows
    vel = (np.float64(state["xd"]) + np.float64(push[0]), np.float64(state["yd"]) + np.float64(push[1]))      # formed once in fp64: data
    t.axes = []
    for axis in (0, 1):
        q = _axis_problem(mp, p, center, state, vel[axis], axis, rows)
        res = _solve_axis(mp, p, q, rows, hint[axis])
        res["q"] = q
        t.axes.append(res)
        if not res["certified"]:
            return t
    t.ok = True
    dt, eta = t.axes[0]["q"]["dt"], t.axes[0]["q"]["eta"]
    ch, sh = mp.cosh(eta * dt), mp.sinh(eta * dt)
    t.u0 = [r["u"][0] for r in t.axes]
    t.f0 = [r["f"][0] for r in t.axes]
    t.com_before = [mpf(float(state["x"])), mpf(float(state["y"]))]
    t.pos, t.vel, t.zmp = [], [], []
    for axis in (0, 1):
        a, b, c, u = t.com_before[axis], mpf(float(vel[axis])), mpf(float(state[("xz", "yz")[axis]])), t.u0[axis]
        t.pos.append(ch * a + sh / eta * b + (1 - ch) * c + (dt - sh / eta) * u)
        t.vel.append(eta * sh * a + ch * b - eta * sh * c + (1 - ch) * u)
        t.zmp.append(c + dt * u)
    t.stepped = j + 1 >= p.step * fc
    t.cur = [mpf(float(state["cur_x"])), mpf(float(state["cur_y"]))]
    t.off = [mpf(float(state["off_x"])), mpf(float(state["off_y"]))]
    t.fc, t.j, t.rebuilt = fc, j + 1, int(state["rebuilt"])
    if t.stepped:
        t.fc, t.rebuilt = fc + 1, 1
        t.cur = list(t.f0)
        t.off = [t.off[ax] + (t.f0[ax] - (mpf(float(center[fc, ax])) + t.off[ax])) for ax in (0, 1)]      # off += f0 - fs[fc + 1]
    t.active = [1 + len(r["W"]) for r in t.axes]
    t.margins = [[r["slack"], r["mult"]] for r in t.axes]
    return t


def kept(t):
    return t.ok and all(m[0] >= MARGIN_SLACK and m[1] >= MARGIN_MULT for m in t.margins)


def _fp64(v):
    """mpf -> fp64, rounded once.  The value is first rounded to 40 digits: the last ten of a solve depend on the route of the refinement,
    and where the exact value is a tie between two fp64 numbers (zmp + dt u0 with row 1 active is a sum of two fp64 numbers) they would
    decide the rounding; at 40 digits a tie is a tie and rounds to even."""
    import mpmath
    with mpmath.workdps(40):
        return float(+v)


def to_records(t):
    """(OUT_A record, STATE_A record after the tick), every number rounded to fp64 once; status 0, iters 0, active = x | y << 16 in the
    kernels' convention (1 for the stability row + active ZMP rows + active kinematic rows per axis)."""
    o, s = np.zeros(1, OUT_A), np.zeros(1, STATE_A)
    o["com_before"][0] = [_fp64(v) for v in t.com_before]; o["vel_after"][0] = [_fp64(v) for v in t.vel]
    o["u0"][0] = [_fp64(v) for v in t.u0]; o["f0"][0] = [_fp64(v) for v in t.f0]
    o["active"][0] = t.active[0] | (t.active[1] << 16)
    for k, v in (("x", t.pos[0]), ("xd", t.vel[0]), ("xz", t.zmp[0]), ("y", t.pos[1]), ("yd", t.vel[1]), ("yz", t.zmp[1]),
                 ("cur_x", t.cur[0]), ("cur_y", t.cur[1]), ("off_x", t.off[0]), ("off_y", t.off[1])):
        s[k][0] = _fp64(v)
    s["fc"][0], s["j"][0], s["rebuilt"][0] = t.fc, t.j, t.rebuilt
    return o[0], s[0]


def tick_arrays(t, width):
    """What a fixture stores of one tick beside the two records: working sets as signs over rows 1 .. C + F, the solutions, multipliers."""
    C, F = t.p.C, t.p.F
    ws, sol, mu = np.zeros((2, width), np.int8), np.zeros((2, width)), np.zeros((2, width + 1))
    for ax, r in enumerate(t.axes):
        for (i, s), m in zip(r["W"], r["mu"][1:]):
            ws[ax, i - 1] = s; mu[ax, i] = _fp64(m)
        mu[ax, 0] = _fp64(r["mu"][0])
        sol[ax, :C + F] = [_fp64(v) for v in r["u"]] + [_fp64(v) for v in r["f"]]
    return dict(ws=ws, sol=sol, mu=mu, margins=np.array([[_fp64(v) for v in m] for m in t.margins]))


# ---- fixtures and the shared comparison (no mpmath below this line) ------------------------------------------------------------------
_groups = {}


def load_group(group):
    """The committed fixture of a group as a dict of arrays (read-only), loaded once."""
    if group not in _groups:
        z = np.load(os.path.join(GOLDEN, f"formA_exact_{group}.npz"))
        d = {k: z[k] for k in z.files}
        for v in d.values():
            v.setflags(write=False)
        _groups[group] = d
    return _groups[group]


def group_floor(fx, key="floor"):
    return {k: float(v) for k, v in zip(QUANTITIES, fx[key])}


def quantities(out, state):
    """The compared quantities of OUT_A records and the STATE_A records after the tick, [n, .] each.  vel holds both copies of the next
    velocity (the record's vel_after and the state's xd, yd)."""
    col = lambda *ks: np.stack([np.asarray(state[k], dtype=np.float64).reshape(-1) for k in ks], 1)
    return dict(u0=np.asarray(out["u0"]).reshape(-1, 2), f0=np.asarray(out["f0"]).reshape(-1, 2), com=col("x", "y"),
                vel=np.concatenate([np.asarray(out["vel_after"]).reshape(-1, 2), col("xd", "yd")], 1), zmp=col("xz", "yz"),
                cur_off=col("cur_x", "cur_y", "off_x", "off_y"), com_before=np.asarray(out["com_before"]).reshape(-1, 2),
                status=np.asarray(out["status"]).reshape(-1), fc=np.asarray(state["fc"]).reshape(-1), j=np.asarray(state["j"]).reshape(-1),
                rebuilt=np.asarray(state["rebuilt"]).reshape(-1))


def errors(got, exact):
    return {k: float(np.abs(got[k] - exact[k]).max()) for k in QUANTITIES}


def reference_floor(e):
    """errors() of a reference-side evaluation as a floor: cur / off is taken as at least the f0 error.  On a tick that switches footsteps
    cur IS f0 (off = f0 - center carries the same error) and on every other tick it is the input, so the reference-side error of cur / off
    is the f0 error sampled on the few switching ticks of a group; the f0 error over all its ticks is the same quantity's better sample."""
    e = dict(e)
    e["cur_off"] = max(e["cur_off"], e["f0"])
    return e


def assert_exact_a(got, exact, floor, factor=BOUND_FACTOR, label=None, same_input=True):
    """got, exact: quantities() of the same ticks; floor: {quantity: bound unit}.  Status, fc, j, rebuilt bit for bit, and so is com_before
    where both sides were given the same state (single ticks; in a closed loop it is the previous tick's `com`, which is compared);
    every quantity, over every tick and both axes, within factor x floor.  Nothing is excluded.  Returns the errors."""
    for k in QUANTITIES:
        assert got[k].shape == exact[k].shape, (label, k, got[k].shape, exact[k].shape)
    e = errors(got, exact)
    if label is not None:
        print(f"exactA[{label}] " + " ".join(f"{k}={e[k]:.3e}/{floor[k]:.3e}" for k in QUANTITIES))
    for k in COUNTERS:
        assert np.array_equal(got[k], exact[k]), (label, k, np.flatnonzero(got[k] != exact[k]))
    assert not same_input or got["com_before"].tobytes() == exact["com_before"].tobytes(), label
    for k in QUANTITIES:
        assert np.isfinite(got[k]).all() and e[k] <= factor * floor[k], (label, k, e[k], floor[k], e[k] / floor[k])
    return e


def fixture_exact(fx, sel=None):
    """quantities() of the fixture's exact records (of ticks `sel`)."""
    out, st = fx["out"].view(OUT_A).reshape(-1), fx["state_after"].view(STATE_A).reshape(-1)
    if sel is not None:
        out, st = out[sel], st[sel]
    return quantities(out, st)


def active_sizes(out):
    """[n, 2] working-set sizes of OUT_A records: x in the low 16 bits, y above."""
    a = np.asarray(out["active"]).reshape(-1)
    return np.stack([a & 0xffff, (a >> 16) & 0xffff], 1)
