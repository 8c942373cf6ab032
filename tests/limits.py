"""Host restatement of the limited closed loops (tolg_policy_rollout_limited): tests/restate.py::restate_policy with the
actuator's clamp, its counts, the excess and the clearance from keep-out spheres, from oracle primitives and numpy only.  A plain
module (pytest does not collect it)."""
import numpy as np

from oracle import bridge as ob


def clamp(u, lb, ub):
    """u < lb ? lb : (u > ub ? ub : u), entry by entry: a NaN stays NaN (neither comparison holds)."""
    u = np.asarray(u, float)
    return np.where(u < lb, lb, np.where(u > ub, ub, u))


def count_and_excess(uc, lb, ub):
    """From commanded inputs uc [..., N, m] and a box lb, ub [m]: (n_sat [...], u_excess [...]) -- the number of entries
    outside the box and max(lb - u, u - ub, 0) over all of them (fmax: a NaN distance is passed over)."""
    uc = np.asarray(uc, float)
    out = (uc < lb) | (uc > ub)
    ex = np.fmax(np.fmax(lb - uc, uc - ub), 0.0)
    return out.sum(axis=(-1, -2)).astype(np.int32), ex.max(axis=(-1, -2))


def clearance_of(t, spheres):
    """t [N+1, 3] positions, spheres [K, 4] (one geometry for every knot) or [N+1, K, 4] (knot i's own), rows (cx, cy, cz, r).
    Returns (min_{i,k} |t_i - c_ik| - r_ik, the first knot that attains it, the smallest of the other knots' own minima): a
    strict < update with knots ascending and spheres ascending, as the kernel runs it."""
    t = np.asarray(t, float)
    sp = np.asarray(spheres, float)
    if sp.ndim == 2:
        sp = np.broadcast_to(sp, (t.shape[0],) + sp.shape)
    best, knot = np.inf, 0
    per_knot = np.full(t.shape[0], np.inf)
    for i in range(t.shape[0]):
        for k in range(sp.shape[1]):
            c = np.sqrt(np.sum((t[i] - sp[i, k, :3]) ** 2)) - sp[i, k, 3]
            per_knot[i] = min(per_knot[i], c) if not np.isnan(c) else per_knot[i]
            if c < best:
                best, knot = c, i
    others = np.delete(per_knot, knot)
    return best, knot, (others.min() if others.size else np.inf)


def restate_policy_limited(op, q_nom, xi_nom, u_nom, K, lb, ub, dx0=None, noise=None, S=1, spheres=None, op_plant=None):
    """S closed-loop rollouts of one trajectory's policy under the box [lb, ub] ([m] each; None: no limit):
    x^_0 = x*_0 (+) dx0, u~_i = u*_i + K_i [x^_i (-) x*_i], u^_i = clamp(u~_i), x^_{i+1} = f(x^_i, u^_i) + twist noise, the
    cost at u^_i.  op_plant (one OracleProblem or a list of S): the steps on a plant, the cost on the model op.
    spheres [K, 4] or [N+1, K, 4]: this trajectory's keep-out spheres, for the clearance.
    Returns a dict: J [S], xs_q [S, N+1, 4, 4], xs_xi [S, N+1, 6], us [S, N, m] (applied), uc [S, N, m] (commanded),
    n_sat [S], u_excess [S] and, with spheres, clearance [S], clearance_knot [S], runner_up [S] (clearance_of)."""
    N, m = u_nom.shape
    lb = np.full(m, -np.inf) if lb is None else np.asarray(lb, float)
    ub = np.full(m, np.inf) if ub is None else np.asarray(ub, float)
    plants = [op] * S if op_plant is None else (op_plant if isinstance(op_plant, (list, tuple)) else [op_plant] * S)
    J = np.zeros(S)
    xs_q = np.zeros((S, N + 1, 4, 4)); xs_xi = np.zeros((S, N + 1, 6)); us = np.zeros((S, N, m)); uc = np.zeros((S, N, m))
    for s in range(S):
        q, xi = np.array(q_nom[0], float), np.array(xi_nom[0], float)
        if dx0 is not None:
            q = q @ ob.se3_exp(dx0[s, :6])
            xi = xi + dx0[s, 6:]
        for i in range(N):
            e = np.r_[ob.rminus(q, q_nom[i]), xi - xi_nom[i]]
            uc[s, i] = u_nom[i] + K[i] @ e
            u = clamp(uc[s, i], lb, ub)
            xs_q[s, i], xs_xi[s, i], us[s, i] = q, xi, u
            J[s] += ob.cost(op, q, xi, u, i)[0]
            q, xi = ob.f(plants[s], q, xi, u)
            if noise is not None:
                xi = xi + noise[s, i]
        xs_q[s, N], xs_xi[s, N] = q, xi
        J[s] += ob.cost(op, q, xi, None, N, terminal=True)[0]
    n_sat, ex = count_and_excess(uc, lb, ub)
    out = dict(J=J, xs_q=xs_q, xs_xi=xs_xi, us=us, uc=uc, n_sat=n_sat, u_excess=ex)
    if spheres is not None:
        c = [clearance_of(xs_q[s, :, :3, 3], spheres) for s in range(S)]
        out.update(clearance=np.array([x[0] for x in c]), clearance_knot=np.array([x[1] for x in c], dtype=np.int32),
                   runner_up=np.array([x[2] for x in c]))
    return out


def box_from_unlimited(u_nom, uc, fin, widen=0.5):
    """The box of the parity tests, from the unlimited restatement of one trajectory: the nominal range of every input over
    the knots, widened by half (`widen`) the largest excursion the finite samples' commands make beyond it.  u_nom [N, m],
    uc [S, N, m], fin [S] bool.  Returns (lb [m], ub [m])."""
    lo, hi = u_nom.min(axis=0), u_nom.max(axis=0)
    exc = np.fmax(np.fmax(lo - uc[fin], uc[fin] - hi), 0.0).max(initial=0.0)
    return lo - widen * exc, hi + widen * exc


def near_bound(uc, lb, ub, tol=1e-8):
    """[S] bool: some commanded input of the sample lies within tol of a bound (its n_sat may differ by rounding)."""
    return ((np.abs(uc - lb) < tol) | (np.abs(uc - ub) < tol)).any(axis=(-1, -2))


def restate_limited_batch(ops, nom, K, dx0, w, box=None, widen=0.5):
    """Per trajectory: the box (given as (lb [B, m], ub [B, m]), or box_from_unlimited on the unlimited restatement) and the
    limited restatement under it.  ops: one OracleProblem per trajectory; nom: xs_q / xs_xi / us [B, ...] (numpy).
    Returns (lb [B, m], ub [B, m], [restate_policy_limited's dict per trajectory])."""
    S = dx0.shape[1]
    lbs, ubs, out = [], [], []
    with np.errstate(all="ignore"):
        for b, op in enumerate(ops):
            a = (op, nom.xs_q[b], nom.xs_xi[b], nom.us[b], K[b])
            if box is None:
                free = restate_policy_limited(*a, None, None, dx0[b], w[b], S)
                lb, ub = box_from_unlimited(nom.us[b], free["uc"], np.isfinite(free["J"]), widen)
            else:
                lb, ub = box[0][b], box[1][b]
            out.append(restate_policy_limited(*a, lb, ub, dx0[b], w[b], S))
            lbs.append(lb); ubs.append(ub)
    return np.array(lbs), np.array(ubs), out
