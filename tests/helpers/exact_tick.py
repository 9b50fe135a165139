"""Test infrastructure: one Formulation B tick (MPCSolver::solve, stage by stage as oracle/ismpc_oracle.c:164-374 lays it out) in exact
arithmetic -- mpmath at DPS digits -- plus the comparison the rounding-level tests share (assert_exact).

The problem data are the fp64 numbers taken as exact: the ismpc_params fields, the tick-in record and the midpoint table as
Oracle.midpoint() returns it (data, not code).  Everything derived (eta, deltas, cosh / sinh, the transition products, the Hessian)
is evaluated in mpmath from those, and the results are rounded to fp64 once, at the end.

It is not a QP solver and shares nothing with the Goldfarb-Idnani or qpOASES code paths: closed forms plus certificates.

  vertical stage   H from the closed forms (S[k][j] = (k-j) dt^2/m, Sv[k][j] = dt/m for j < k), inverted once per parameter set.  The
                   equality set follows mpc_iter, S, F and footstep_counter > 1.  The working set of the rows z_lo <= S u <= z_hi starts
                   empty; if a row is violated the candidate set is read off a hint (the fp64 oracle's trajectory: rows within 1e-9 of a
                   bound).  The equality-constrained problem is solved exactly and CERTIFIED: every row feasible, every multiplier of
                   the right sign, complementarity strict.  The smallest margin is returned.
  stage 2          lambda_j for every j, and the branch margin min_j |lambda_j - gate| / gate.
  stage 3          a, beq (with the anticipative tail), the box mid +- half; u = clip(mid + nu a, lo, hi) with nu the root of the monotone
                   piecewise-linear a'u(nu) = beq, found by sorting the breakpoints.  Infeasible exactly when beq lies outside the range
                   of a'u over the box.

mpmath is imported when a tick is computed, not when this module is: assert_exact and the fixture loader run without it.
"""
import os

import numpy as np

DPS = 50
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
ST_X_INFEASIBLE, ST_Y_INFEASIBLE, ST_Z_INEQ_ACTIVE, ST_BAD_INDEX, ST_FLIGHT, ST_TICK_SKIPPED = 1, 2, 4, 8, 16, 32
QUANTITIES = ("u_z", "u_x", "u_y", "u0", "com_pos", "com_vel")
BOUND_FACTOR = 16          # four bits over a plain fp64 dense evaluation (the stored floor): summation order, table precision
HINT_BAND = 1e-9           # rows of the hint within this distance of a bound form the candidate working set
PARAM_FIELDS = ("N", "S", "F", "M", "mpc_dt", "control_dt", "mass", "g", "h_des", "foot_width", "first_step_halfwidth", "q_p", "q_u", "q_v",
                "z_ineq_lo", "z_ineq_hi", "lambda_gate")

_hinv = {}


def params_key(p):
    return tuple(getattr(p, k) for k in PARAM_FIELDS)


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def hessian_inverse(p):
    """(H^-1 as a list of rows, mpf), cached per parameter set.  H = q_p S'S + q_v Sv'Sv + q_u I with integer-valued sums in closed form."""
    key = params_key(p)
    if key in _hinv:
        return _hinv[key]
    mp = _mp()
    mpf, fdot = mp.mpf, mp.fdot
    N = p.N
    dt, m = mpf(p.mpc_dt), mpf(p.mass)
    cp, cv, qu = mpf(p.q_p) * (dt * dt / m) ** 2, mpf(p.q_v) * (dt / m) ** 2, mpf(p.q_u)

    def pair(i, j):                                # sum_{k > max(i, j)} (k - i)(k - j), an integer
        return sum((k - i) * (k - j) for k in range(max(i, j) + 1, N))
    H = [[cp * pair(i, j) + cv * (N - 1 - max(i, j)) + (qu if i == j else 0) for j in range(N)] for i in range(N)]
    L = [[mpf(0)] * N for _ in range(N)]           # Cholesky, lower
    for i in range(N):
        for j in range(i + 1):
            s = H[i][j] - fdot(L[i][:j], L[j][:j])
            L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
    XT = [[mpf(0)] * N for _ in range(N)]          # XT[j][i] = (L^-1)[i][j]
    for j in range(N):
        col = XT[j]
        col[j] = 1 / L[j][j]
        for i in range(j + 1, N):
            col[i] = -fdot(L[i][j:i], col[j:i]) / L[i][i]
    Hi = [[None] * N for _ in range(N)]
    for a in range(N):
        for b in range(a + 1):
            Hi[a][b] = Hi[b][a] = fdot(XT[a][a:], XT[b][a:])
    _hinv[key] = (H, Hi)
    return _hinv[key]


def equality_columns(p, mpc_iter, footstep_counter):
    """Columns c with u_c = 0, as oracle/ismpc_oracle.c:189-232 stacks them (rows that fall outside the horizon are dropped there)."""
    N, S, F = p.N, p.S, p.F
    if footstep_counter <= 1:
        return []
    if mpc_iter < S:
        return [i - mpc_iter for i in range(S, min(S + F, N)) if 0 <= i - mpc_iter < N]      # (the loop there runs over i < N)
    return [i for i in range(min(N, max(0, S + F - mpc_iter)))]


class ExactTick:
    """Everything one exact tick produced; fp64 views are rounded once from the mpf values."""
    pass


def _solve_vertical(mp, p, Hi, f, E, W):
    """min 1/2 u'Hu + f'u  s.t.  u_c = 0 (c in E),  S_k u = bound (k, bound in W).  Returns (u, mu_eq {c: mu}, mu_in {k: mu})."""
    mpf, fdot = mp.mpf, mp.fdot
    N = p.N
    c2 = mpf(p.mpc_dt) ** 2 / mpf(p.mass)
    rows = [[mpf(1) if j == c else mpf(0) for j in range(N)] for c in E] + [[c2 * (k - j) if j < k else mpf(0) for j in range(N)] for k, _ in W]
    d = [mpf(0)] * len(E) + [mpf(b) for _, b in W]
    u0 = [-fdot(Hi[i], f) for i in range(N)]
    if not rows:
        return u0, {}, {}
    HiC = [[fdot(Hi[i], r) for i in range(N)] for r in rows]                  # H^-1 C' by column
    G = mp.matrix(len(rows), len(rows))
    rhs = mp.matrix(len(rows), 1)
    for a, ra in enumerate(rows):
        for b in range(len(rows)):
            G[a, b] = fdot(ra, HiC[b])
        rhs[a] = fdot(ra, u0) - d[a]
    mu = mp.lu_solve(G, rhs)
    u = [u0[i] - sum(HiC[a][i] * mu[a] for a in range(len(rows))) for i in range(N)]
    for c in E:
        u[c] = mpf(0)                                                      # exactly: the solve leaves 1e-DPS there
    # (so do active rows that pin leading samples: S_1 u = ... = S_k u = 0 means u_0 = ... = u_{k-1} = 0.  The solve carries DPS digits;
    # a component below 1e-30 of the largest is that residue and is set to the zero it stands for)
    big = max(abs(v) for v in u)
    u = [v if abs(v) > big * mpf(10) ** (20 - DPS) else mpf(0) for v in u]
    return u, {c: mu[a] for a, c in enumerate(E)}, {k: mu[len(E) + a] for a, (k, _) in enumerate(W)}


def exact_tick(p, mid, rec, hint_uz=None):
    """One tick.  p: a Params structure (its fields are read, nothing else); mid: the midpoint table [rows, 3]; rec: one TICK_IN record;
    hint_uz: the fp64 oracle's vertical trajectory, consulted only when a row z_lo <= S u <= z_hi is violated with the empty working set."""
    mp = _mp()
    mpf, fdot = mp.mpf, mp.fdot
    N, S, F = p.N, p.S, p.F
    t = ExactTick()
    t.N = N
    pos, vel = [mpf(float(v)) for v in rec["com_pos"]], [mpf(float(v)) for v in rec["com_vel"]]
    t.com_pos, t.com_vel, t.u0 = list(pos), list(vel), [mpf(0)] * 3
    t.u = [[mpf(0)] * N for _ in range(3)]
    t.status = 0
    t.E, t.W, t.mu_eq, t.mu_in = [], [], {}, {}
    t.lam, t.a, t.beq, t.nu, t.clamped = [mpf(0)] * N, [mpf(0)] * N, [mpf(0)] * 2, [mpf(0)] * 2, [0, 0]
    t.margin_z, t.margin_lam, t.margin_feas = mp.inf, mp.inf, [mp.inf, mp.inf]
    # the two gates are integer decisions on fp64 data: taken as the oracle takes them (oracle/ismpc_oracle.c:180-186)
    divisor = int(100 * p.mpc_dt)
    if divisor <= 0 or int(rec["control_iter"]) % divisor != 0:
        t.status |= ST_TICK_SKIPPED
        return t
    idx = int(float(rec["simulation_time"]) / (p.mpc_dt / p.control_dt))
    if idx < 0 or idx + 2 * N > len(mid) or int(rec["mpc_iter"]) < 0:
        t.status |= ST_BAD_INDEX
        return t
    dt, m, g, h_des = mpf(p.mpc_dt), mpf(p.mass), mpf(p.g), mpf(p.h_des)
    eta = mp.sqrt(g / h_des)
    midz = [[mpf(float(mid[idx + k, c])) for k in range(2 * N)] for c in range(3)]

    # ---- vertical stage
    H, Hi = hessian_inverse(p)
    rp = [pos[2] + (k + 1) * dt * vel[2] - g * dt * dt * (k * (k + 1) // 2) - h_des - midz[2][k] for k in range(N)]
    rv = [vel[2] - g * dt * k for k in range(N)]
    a1 = a2 = b1 = mpf(0)
    f = [None] * N
    for i in range(N - 1, -1, -1):                   # a1 = sum_{k>i} rp[k], a2 = sum_{k>i} (k-i) rp[k], b1 = sum_{k>i} rv[k]
        f[i] = mpf(p.q_p) * (dt * dt / m) * a2 + mpf(p.q_v) * (dt / m) * b1 - mpf(p.q_u) * m * g
        a1 += rp[i]; a2 += a1; b1 += rv[i]
    E = equality_columns(p, int(rec["mpc_iter"]), int(rec["footstep_counter"]))
    free0 = next((j for j in range(N) if j not in E), N)     # rows k <= free0 of S are zero on the free columns: implied by the equalities
    c2 = dt * dt / m
    lo, hi = mpf(p.z_ineq_lo), mpf(p.z_ineq_hi)

    def row_values(u):
        s0 = s1 = mpf(0)
        out = [mpf(0)] * N
        for k in range(1, N):                        # S_k u = c2 sum_{j<k} (k-j) u_j
            s0 += u[k - 1]; s1 += s0
            out[k] = c2 * s1
        return out
    u, mu_eq, mu_in = _solve_vertical(mp, p, Hi, f, E, [])
    W = []
    sv = row_values(u)
    if any(sv[k] < lo or sv[k] > hi for k in range(free0 + 1, N)):
        assert hint_uz is not None, "a vertical row is violated and no hint was given"
        hv = row_values([mpf(float(v)) for v in hint_uz])
        W = [(k, p.z_ineq_lo) for k in range(free0 + 1, N) if abs(hv[k] - lo) <= HINT_BAND] + \
            [(k, p.z_ineq_hi) for k in range(free0 + 1, N) if abs(hv[k] - hi) <= HINT_BAND]
        W.sort()
        u, mu_eq, mu_in = _solve_vertical(mp, p, Hi, f, E, W)
        sv = row_values(u)
    # the certificate: inactive rows strictly inside (slack in metres), multipliers of active rows strictly of the right sign (relative to
    # the gradient's scale m g q_u); zero rows (k <= free0) hold for every u as long as lo <= 0 <= hi
    active = dict(W)
    gscale = mpf(p.q_u) * m * g
    margin = mp.inf
    for k in range(free0 + 1, N):
        if k in active:
            s = mu_in[k] if active[k] == p.z_ineq_hi else -mu_in[k]         # upper row active: mu > 0; lower: mu < 0
            margin = min(margin, s / gscale)
        else:
            margin = min(margin, sv[k] - lo, hi - sv[k])
    if not (lo <= 0 <= hi):
        margin = -mp.inf
    t.margin_z = margin
    t.E, t.W, t.mu_eq, t.mu_in = E, W, mu_eq, mu_in
    t.f = f
    if W:
        t.status |= ST_Z_INEQ_ACTIVE
    t.u[0] = u
    t.com_pos[2] = pos[2] + dt * vel[2]
    t.com_vel[2] = vel[2] + dt / m * u[0] - dt * g
    t.u0[0] = u[0]

    # ---- stage 2
    gate = mpf(p.lambda_gate)
    lam = [None] * N
    for j in range(N):
        zpos = sv[j] + pos[2] + (j + 1) * dt * vel[2] - g * dt * dt * (j * (j + 1) // 2)
        lam[j] = (u[j] / m) / zpos
    t.lam = lam
    t.margin_lam = min(abs(l - gate) for l in lam) / gate

    def AB(l):
        if l < gate:
            return (mpf(1), dt, mpf(0), mpf(1)), (mpf(0), mpf(0))
        sq = mp.sqrt(l)
        ch, sh = mp.cosh(sq * dt), mp.sinh(sq * dt)
        return (ch, sh / sq, sq * sh, ch), (1 - ch, -sq * sh)

    # ---- stage 3
    if lam[0] > gate:
        half = mpf(p.foot_width) / 2 if int(rec["footstep_counter"]) > 1 else mpf(p.first_step_halfwidth)
        r = (mpf(1), 1 / eta)                                # C_sc A_{N-1} ... A_{i+1}
        a = [None] * N
        for i in range(N - 1, -1, -1):
            A, B = AB(lam[i])
            a[i] = r[0] * B[0] + r[1] * B[1]
            r = (r[0] * A[0] + r[1] * A[2], r[0] * A[1] + r[1] * A[3])
        t.a = a
        w = [eta * dt * mp.exp(-dt * eta * i) for i in range(N)]
        absa = [abs(v) for v in a]
        cap = half * mp.fsum(absa)
        order = sorted((i for i in range(N) if absa[i] != 0), key=lambda i: half / absa[i])
        for ax, s in ((0, (pos[0], vel[0])), (1, (pos[1], vel[1]))):
            beq = -(r[0] * s[0] + r[1] * s[1]) + fdot(w, midz[ax][N:2 * N])
            t.beq[ax] = beq
            tgt = beq - fdot(a, midz[ax][:N])
            t.margin_feas[ax] = (cap - abs(tgt)) / cap
            if abs(tgt) > cap:
                t.status |= (ST_X_INFEASIBLE, ST_Y_INFEASIBLE)[ax]
                continue
            # g(nu) = half sum_{clamped} |a_i| + nu sum_{free} a_i^2 on nu >= 0, breakpoints half / |a_i| ascending
            sat, rest, k = mpf(0), mp.fsum(v * v for v in absa), 0
            nu = abs(tgt) / rest
            while k < len(order) and nu * absa[order[k]] > half:
                i = order[k]
                sat += half * absa[i]; rest -= absa[i] ** 2; k += 1
                nu = (abs(tgt) - sat) / rest
            nu = nu if tgt >= 0 else -nu
            t.nu[ax], t.clamped[ax] = nu, k
            t.u[1 + ax] = [midz[ax][i] + max(-half, min(half, nu * a[i])) for i in range(N)]
    else:
        t.status |= ST_FLIGHT
    A, B = AB(lam[0])
    for ax in (0, 1):
        z0 = t.u[1 + ax][0]
        t.com_pos[ax] = A[0] * pos[ax] + A[1] * vel[ax] + B[0] * z0
        t.com_vel[ax] = A[2] * pos[ax] + A[3] * vel[ax] + B[1] * z0
        t.u0[1 + ax] = z0
    return t


def certified(t, band=1e-9):
    """The conditions under which an instance enters a fixture: vertical strict complementarity, every lambda_j away from the gate, both
    horizontal QPs away from their feasibility boundary (the band the project uses for it)."""
    if t.status & (ST_TICK_SKIPPED | ST_BAD_INDEX):
        return True
    if not (t.margin_z > band and t.margin_lam > band):
        return False
    return bool(t.status & ST_FLIGHT) or all(abs(v) > band for v in t.margin_feas)


def to_fp64(t):
    """(out fields dict, u_traj [3, N]) rounded once."""
    f = lambda v: np.array([float(x) for x in v])
    return dict(com_pos=f(t.com_pos), com_vel=f(t.com_vel), u0=f(t.u0), status=np.int32(t.status)), np.stack([f(t.u[0]), f(t.u[1]), f(t.u[2])])


def instance_arrays(t):
    """What a fixture stores of one instance, every number rounded to fp64 once."""
    N = t.N
    o, traj = to_fp64(t)
    rec = np.zeros(1, dtype=TICK_OUT)
    for k in ("com_pos", "com_vel", "u0", "status"):
        rec[k][0] = o[k]
    eq_mask = np.zeros(N, bool); eq_mask[t.E] = True
    mu_eq, mu_in, w_sign = np.zeros(N), np.zeros(N), np.zeros(N, np.int8)
    for c, v in t.mu_eq.items():
        mu_eq[c] = float(v)
    for k, v in t.mu_in.items():
        mu_in[k] = float(v)
    for k, b in t.W:
        w_sign[k] = 1 if float(mu_in[k]) > 0 else -1
    fin = lambda v: float(v)
    return dict(tick_out=rec.view(np.uint8).reshape(-1), u_traj=traj, lambda0=fin(t.lam[0]), beq=np.array([fin(v) for v in t.beq]),
                nu=np.array([fin(v) for v in t.nu]), clamped=np.array(t.clamped, np.int32), eq_mask=eq_mask, mu_eq=mu_eq, w_sign=w_sign, mu_in=mu_in,
                margins=np.array([fin(t.margin_z), fin(t.margin_lam), fin(t.margin_feas[0]), fin(t.margin_feas[1])]))


def exact_rollout(p, mid, orc, state, first_frame, ticks):
    """The exact tick applied tick by tick.  The integer bookkeeping fields and the frame time come from the oracle's rollout inputs (they
    depend on the frame alone); the exact state is rounded to fp64 at every tick, as the kernels store it.  Returns (input records, exact
    output records, the oracle's own rollout, all ticks certified)."""
    ref, ins, _, _ = orc.rollout(state, first_frame, ticks)
    ins = ins.copy()
    outs = np.zeros(ticks, dtype=TICK_OUT)
    pos, vel = np.array(state["com_pos"]).reshape(3).copy(), np.array(state["com_vel"]).reshape(3).copy()
    ok = True
    for k in range(ticks):
        ins["com_pos"][k], ins["com_vel"][k] = pos, vel
        hint = orc.solve(ins[k:k + 1], want_traj=True)[2][0, 0]
        t = exact_tick(p, mid, ins[k], hint)
        ok = ok and certified(t) and not (t.status & (ST_X_INFEASIBLE | ST_Y_INFEASIBLE))
        o, _ = to_fp64(t)
        for f in ("com_pos", "com_vel", "u0", "status"):
            outs[f][k] = o[f]
        pos, vel = o["com_pos"], o["com_vel"]
    return ins, outs, ref, ok


# ---- fixtures and the shared comparison (no mpmath below this line) ------------------------------------------------------------------
_groups = {}


def load_group(group):
    """The committed fixture of a group as a dict of arrays (read-only), loaded once."""
    if group not in _groups:
        z = np.load(os.path.join(GOLDEN, f"formB_exact_{group}.npz"))
        d = {k: z[k] for k in z.files}
        for v in d.values():
            v.setflags(write=False)
        _groups[group] = d
    return _groups[group]


def group_floor(fx, prefix="floor"):
    return {k: float(v) for k, v in zip(QUANTITIES, fx[prefix])}


def errors(out, traj, ref_out, ref_traj):
    """Largest absolute error per quantity.  The horizontal quantities of an instance with an infeasible horizontal QP are left out (status
    only: there is no solution to compare); its vertical ones stay in."""
    inf = (ref_out["status"] & (ST_X_INFEASIBLE | ST_Y_INFEASIBLE)) != 0
    okh = ~inf
    e = {}
    e["u_z"] = float(np.abs(traj[:, 0] - ref_traj[:, 0]).max())
    e["u_x"] = float(np.abs(traj[okh, 1] - ref_traj[okh, 1]).max()) if okh.any() else 0.0
    e["u_y"] = float(np.abs(traj[okh, 2] - ref_traj[okh, 2]).max()) if okh.any() else 0.0
    for k in ("u0", "com_pos", "com_vel"):
        d = np.abs(out[k] - ref_out[k])
        horiz = slice(1, 3) if k == "u0" else slice(0, 2)          # u0 = (force, ZMP x, ZMP y); the CoM fields are (x, y, z)
        d[inf, horiz] = 0.0
        e[k] = float(d.max())
    return e


def assert_exact(out, traj, group, sel=None, floor="floor", label=None):
    """out: TICK_OUT records, traj: [B, 3, N] decision trajectories of the fixture's instances (or of fixture instances `sel`), against the
    exact values: status bit for bit, every quantity within BOUND_FACTOR x the group's stored floor (the fp64 oracle's own error against
    the same exact values).  Returns the measured errors; prints them when a label is given."""
    fx = load_group(group)
    ref_out = fx["tick_out"].view(TICK_OUT).reshape(-1)
    ref_traj = fx["u_traj"]
    if sel is not None:
        ref_out, ref_traj = ref_out[sel], ref_traj[sel]
    assert len(out) == len(ref_out) and traj.shape == ref_traj.shape, (len(out), traj.shape, ref_traj.shape)
    e = errors(out, traj, ref_out, ref_traj)
    fl = group_floor(fx, floor)
    if label is not None:
        print(f"exact[{label}] " + " ".join(f"{k}={e[k]:.3e}/{fl[k]:.3e}" for k in QUANTITIES))
    assert np.array_equal(out["status"], ref_out["status"]), (group, np.flatnonzero(out["status"] != ref_out["status"]))
    for k in QUANTITIES:
        assert e[k] <= BOUND_FACTOR * fl[k], (group, label, k, e[k], fl[k])
    return e


ROLL_QUANTITIES = ("u0", "com_pos", "com_vel")


def assert_exact_rollout(out, group, j, label=None):
    """out: the TICK_OUT records of closed-loop instance j of the group, tick by tick, against the exact tick applied tick by tick; the
    floor is the fp64 oracle's own rollout against that exact rollout."""
    fx = load_group(group)
    ref = fx["roll_out"][j].view(TICK_OUT).reshape(-1)
    assert len(out) == len(ref)
    e = {k: float(np.abs(out[k] - ref[k]).max()) for k in ROLL_QUANTITIES}
    fl = {k: float(v) for k, v in zip(ROLL_QUANTITIES, fx["roll_floor"])}
    if label is not None:
        print(f"exact[{label}] " + " ".join(f"{k}={e[k]:.3e}/{fl[k]:.3e}" for k in ROLL_QUANTITIES))
    assert np.array_equal(out["status"], ref["status"]), (group, j, out["status"], ref["status"])
    for k in ROLL_QUANTITIES:
        assert e[k] <= BOUND_FACTOR * fl[k], (group, j, label, k, e[k], fl[k])
    return e


TICK_IN = np.dtype([("com_pos", "<f8", 3), ("com_vel", "<f8", 3), ("simulation_time", "<f8"), ("mpc_iter", "<i4"), ("control_iter", "<i4"),
                    ("footstep_counter", "<i4"), ("reserved", "<i4")], align=False)
TICK_OUT = np.dtype([("com_pos", "<f8", 3), ("com_vel", "<f8", 3), ("u0", "<f8", 3), ("status", "<i4"), ("iters", "<i4")], align=False)
