"""Test infrastructure: an independent reference of the swing-foot re-placement (the scripts' second quadprog), numpy only.

Written from the description of the step, not from the oracle's C: the target is computed in numpy.longdouble and the QP
    min 1/2 |X - target|^2   s.t.   A X <= b
is solved AS a QP, by enumerating the subsets of its 6 (trot) or 3 (walk) rows, solving each subset's KKT system and keeping the
primal- and dual-feasible candidate of least cost.  Nothing here knows that A happens to describe a box, so it checks the closed
form ("project the target on the box") that both the device kernel and the oracle use.

Plans are [rows, 8] arrays, columns BL, BR, FR, FL as xy; `fc` is the 1-based footstep counter the tick ran with, so plan row fc of
the scripts is plan[fc - 1] here."""
import itertools

import numpy as np

TROT, WALK = 0, 1
BL, BR, FR, FL = 0, 2, 4, 6                      # first (x) column of each foot
LEFT = (BL, FL)                                  # left feet have their outer side up: y in [p_y - disp_i, p_y + disp_o]
FEET_PAD = 8                                     # rows behind the plan that the step may write (ISMPC_A_FEET_PAD)
LD = np.longdouble
EPS = 2e-15                                      # feasibility / activity threshold of the enumeration [m]: rounding of a KKT solve on metre-sized data

# walk: fc -> (moving foot, the fixed diagonal); trot: parity -> (moving feet in the scripts' order of unknowns, fixed diagonal)
WALK_RULE = {2: (FL, (BL, FR)), 4: (BR, (BL, FR)), 6: (FR, (BR, FL)), 8: (BL, (BR, FL))}
TROT_RULE = {1: ((BL, FR), (BR, FL)), 0: ((FL, BR), (BL, FR))}


def replaces(fc, plan_rows):
    """The end-of-plan rule of include/ismpc_a.h: with plan_rows plan rows (the block holds plan_rows + FEET_PAD), the step
    re-places feet for 1 <= fc <= plan_rows - 1 and leaves the block alone otherwise."""
    return 1 <= fc <= plan_rows - 1


def moving_feet(gait, fc):
    """Columns of the feet the step at fc moves, in the order of the QP's unknowns; () when it moves none."""
    if gait == TROT:
        return TROT_RULE[fc % 2][0]
    return (WALK_RULE[fc][0],) if fc in WALK_RULE else ()


def first_step(gait, fc):
    """The scripts' "dummy" steps, whose three limits are halved."""
    return fc == 1 if gait == TROT else fc in (2, 4)


def solve_qp(target, A, b):
    """min 1/2 |X - target|^2 s.t. A X <= b by enumeration of the active sets.  Returns (X, active [rows of A] bool)."""
    n, best = len(target), None
    for k in range(A.shape[0] + 1):
        for S in itertools.combinations(range(A.shape[0]), k):
            S = list(S)
            if k and np.linalg.matrix_rank(A[S]) < k:
                continue                                            # dependent rows: the KKT matrix is singular
            K = np.zeros((n + k, n + k)); K[:n, :n] = np.eye(n); K[:n, n:] = A[S].T; K[n:, :n] = A[S]
            try:
                sol = np.linalg.solve(K, np.concatenate([target, b[S]]))
            except np.linalg.LinAlgError:
                continue
            X, lam = sol[:n], sol[n:]
            if (A @ X - b > EPS).any() or (lam < -EPS).any():
                continue
            cost = 0.5 * float((X - target) @ (X - target))
            if best is None or cost < best[0]:
                best = (cost, X)
    assert best is not None, "the foot QP has no feasible active set"
    X = best[1]
    return X, (b - A @ X) <= EPS


def _line_targets(phi, m, z, anchors):
    """Trot: the opposite-slope line through z (slope -m) cut by the line of slope tan(phi) through each anchor."""
    zx, zy = z
    out = []
    for ax, ay in anchors:
        if phi == np.pi / 2:
            x = ax; y = zy - m * (x - zx)
        else:
            tp = np.tan(LD(phi))
            x = (zy + m * zx - ay + tp * ax) / (tp + m); y = tp * (x - ax) + ay
        out += [x, y]
    return out


def displacement(gait, fc, z, plan):
    """d = z - (the line through the two fixed feet of row fc, cut by the line of opposite slope through z), in long double, with the
    slope m of the fixed diagonal, the scripts' decision `d != 0` and whether that decision is a tie.

    The scripts take the decision on doubles: the intersection is solved symbolically, i.e. exactly, converted to double and subtracted
    from z.  So `changed` is decided here on the long-double intersection ROUNDED to double.  When the tick's QP pins the predicted
    footstep to the fixed diagonal, d is zero up to the rounding of z itself (1e-18 m was seen) and the exact test `d != 0` is decided by
    the last bit of whatever arithmetic evaluates it: such a step is a TIE (|d| within 8 ulp of the coordinates on both axes), and both
    outcomes -- the re-placed target and the planned one, each followed by the same QP -- are answers of the scripts' rule."""
    mov = moving_feet(gait, fc)
    fix = TROT_RULE[fc % 2][1] if gait == TROT else WALK_RULE[fc][1]
    P = np.asarray(plan, dtype=np.float64).astype(LD)
    zx, zy = LD(z[0]), LD(z[1])
    (f1x, f1y), (f2x, f2y) = [(P[fc - 1, c], P[fc - 1, c + 1]) for c in fix]
    m = (f2y - f1y) / (f2x - f1x); q = f1y - m * f1x                      # the line through the two fixed feet of row fc
    xi = (zy + m * zx - q) / (2 * m); yi = m * xi + q                     # cut by the line of slope -m through z
    d = (zx - xi, zy - yi)
    changed = bool(np.float64(z[0]) != np.float64(xi) or np.float64(z[1]) != np.float64(yi))
    ulp = 8 * np.finfo(np.float64).eps
    tie = bool(abs(d[0]) <= ulp * max(abs(zx), abs(xi)) and abs(d[1]) <= ulp * max(abs(zy), abs(yi)))
    return d, m, changed, tie, mov, fix


def feet_step(gait, phi, disp_i, disp_o, disp_forw, fc, z, plan, changed=None):
    """One swing-foot step.  Returns (plan after, active): active is a bool array over the QP's rows -- per moving foot
    [y <= upper, -y <= -lower, x <= forward], feet in the scripts' order of unknowns -- or None when the step moves no foot
    (walk at an fc other than 2, 4, 6, 8).  changed: None takes the scripts' decision `d != 0` as displacement() does; True / False
    force it (the other answer of a tie)."""
    plan = np.array(plan, dtype=np.float64)
    assert plan.ndim == 2 and plan.shape[1] == 8 and fc >= 1 and fc + FEET_PAD <= plan.shape[0], "the step would leave the block"
    if not moving_feet(gait, fc):
        return plan, None
    d, m, decided, _, mov, fix = displacement(gait, fc, z, plan)
    changed = decided if changed is None else changed
    r0, r1 = fc - 1, fc                                                   # rows fc and fc+1 of the scripts
    P = plan.astype(LD)
    zx, zy = LD(z[0]), LD(z[1])
    if gait == TROT:
        if changed:
            target = _line_targets(phi, m, (zx, zy), [(P[r1, c], P[r1, c + 1]) for c in mov])
            for c in fix:
                plan[r1, c:c + 2] = plan[r0, c:c + 2]
        else:
            target = [P[r1, c + k] for c in mov for k in (0, 1)]
    else:
        c = mov[0]
        target = [P[r1, c] + d[0], P[r1, c + 1] + d[1]] if changed else [P[r1, c], P[r1, c + 1]]
        if changed:
            plan[r1:r1 + 8, c] = np.float64(target[0]); plan[r1:r1 + 8, c + 1] = np.float64(target[1])
    target = np.array([np.float64(t) for t in target])
    half = 0.5 if first_step(gait, fc) else 1.0
    li, lo, lf = disp_i * half, disp_o * half, disp_forw * half
    nf = len(mov)
    A = np.zeros((3 * nf, 2 * nf)); b = np.zeros(3 * nf)
    for k, c in enumerate(mov):
        px, py = plan[r0, c], plan[r0, c + 1]
        up, dn = (lo, li) if c in LEFT else (li, lo)
        A[3 * k, 2 * k + 1] = 1;      b[3 * k] = py + up
        A[3 * k + 1, 2 * k + 1] = -1; b[3 * k + 1] = -(py - dn)
        A[3 * k + 2, 2 * k] = 1;      b[3 * k + 2] = px + lf
    X, active = solve_qp(target, A, b)
    if gait == TROT:
        for k, c in enumerate(mov):
            plan[r1, c:c + 2] = X[2 * k:2 * k + 2]
    else:
        c = mov[0]
        plan[r1:r1 + 8, c] = X[0]
        if fc == 8:
            plan[r1, c + 1] = X[1]                                        # the scripts write y back to row fc+1 only
        else:
            plan[r1:r1 + 8, c + 1] = X[1]
    return plan, active


def step_error(got, gait, phi, disp_i, disp_o, disp_forw, fc, z, plan):
    """max |got - feet_step(...)| over all entries, the QP's active rows, and whether the step was a tie of `d != 0` (displacement):
    a tie is compared with both of its answers and the nearer one counts."""
    ref, act = feet_step(gait, phi, disp_i, disp_o, disp_forw, fc, z, plan)
    err, tie = float(np.abs(got - ref).max()), False
    if act is not None:
        _, _, decided, tie, _, _ = displacement(gait, fc, z, plan)
        if tie:
            alt, act2 = feet_step(gait, phi, disp_i, disp_o, disp_forw, fc, z, plan, changed=not decided)
            e2 = float(np.abs(got - alt).max())
            if e2 < err:
                err, ref, act = e2, alt, act2
    return err, ref, act, tie
