"""Host restatement of the actuated closed loops (tolg_policy_rollout_actuated, tolg_mpc_advance_actuated): the actuator model
of include/tolg.h stated in a loop -- transport delay, box, first-order lag, rate limit -- around the oracle's dynamics and cost,
from oracle primitives and numpy only, in the style of tests/limits.py::restate_policy_limited.  A plain module (pytest does not
collect it)."""
import numpy as np

from oracle import bridge as ob
from tests.limits import clamp


def actuate(d, a_prev, lb, ub, beta, du):
    """One knot of the model behind the delay line, entry by entry: the box on the delayed command d, the lag towards it from
    the last applied input a_prev, the rate limit.  Returns (applied [m], moved by the rate limit [m] bool)."""
    s = clamp(d, lb, ub)
    l = s - beta * (s - a_prev)
    dl = l - a_prev
    up, dn = dl > du, dl < -du
    return np.where(up, a_prev + du, np.where(dn, a_prev - du, l)), up | dn


def _rows(m, lb, ub, beta, du):
    return (np.full(m, -np.inf) if lb is None else np.asarray(lb, float), np.full(m, np.inf) if ub is None else np.asarray(ub, float),
            np.zeros(m) if beta is None else np.asarray(beta, float), np.full(m, np.inf) if du is None else np.asarray(du, float))


def restate_policy_actuated(op, q_nom, xi_nom, u_nom, K, lb=None, ub=None, beta=None, du=None, delay=0, u_init=None, dx0=None,
                            noise=None, S=1, op_plant=None):
    """S closed-loop rollouts of one trajectory's policy behind the actuator: c_i = u*_i + K_i e_i; d_i = c_{i-delay}, u_init
    ahead of knot `delay`; a_i = actuate(d_i, a_{i-1}) with a_{-1} = u_init (None: u*_0); x_{i+1} = f(x_i, a_i) + twist noise, the
    cost at a_i.  lb, ub, beta, du [m] (None: no box, no lag, no rate limit).  op_plant: one OracleProblem or a list of S.
    Returns a dict: J [S], xs_q, xs_xi, us [S, N, m] (applied), uc [S, N, m] (commanded), ud [S, N, m] (delayed), n_sat [S],
    u_excess [S] (both on ud), n_rate [S], u_gap [S], moved [S, N, m] bool (by the rate limit), a0 [m] (the u_init used)."""
    N, m = u_nom.shape
    lb, ub, beta, du = _rows(m, lb, ub, beta, du)
    u_init = np.array(u_nom[0], float) if u_init is None else np.asarray(u_init, float)
    plants = [op] * S if op_plant is None else (op_plant if isinstance(op_plant, (list, tuple)) else [op_plant] * S)
    J = np.zeros(S)
    xs_q = np.zeros((S, N + 1, 4, 4)); xs_xi = np.zeros((S, N + 1, 6))
    us = np.zeros((S, N, m)); uc = np.zeros((S, N, m)); ud = np.zeros((S, N, m)); moved = np.zeros((S, N, m), bool)
    for s in range(S):
        q, xi = np.array(q_nom[0], float), np.array(xi_nom[0], float)
        if dx0 is not None:
            q = q @ ob.se3_exp(dx0[s, :6])
            xi = xi + dx0[s, 6:]
        a = u_init.copy()
        for i in range(N):
            e = np.r_[ob.rminus(q, q_nom[i]), xi - xi_nom[i]]
            uc[s, i] = u_nom[i] + K[i] @ e
            ud[s, i] = uc[s, i - delay] if i >= delay else u_init
            a, moved[s, i] = actuate(ud[s, i], a, lb, ub, beta, du)
            xs_q[s, i], xs_xi[s, i], us[s, i] = q, xi, a
            J[s] += ob.cost(op, q, xi, a, i)[0]
            q, xi = ob.f(plants[s], q, xi, a)
            if noise is not None:
                xi = xi + noise[s, i]
        xs_q[s, N], xs_xi[s, N] = q, xi
        J[s] += ob.cost(op, q, xi, None, N, terminal=True)[0]
    out = (ud < lb) | (ud > ub)
    ex = np.fmax(np.fmax(lb - ud, ud - ub), 0.0)
    gap = np.zeros(S)
    for s in range(S):  # fmax: a NaN distance is passed over
        for v in np.abs(us[s] - uc[s]).ravel():
            gap[s] = np.fmax(gap[s], v)
    return dict(J=J, xs_q=xs_q, xs_xi=xs_xi, us=us, uc=uc, ud=ud, n_sat=out.sum(axis=(-1, -2)).astype(np.int32),
                u_excess=ex.max(axis=(-1, -2)), n_rate=moved.sum(axis=(-1, -2)).astype(np.int32), u_gap=gap, moved=moved,
                a0=u_init)


def edge_distance(R, lb=None, ub=None, beta=None, du=None):
    """How close the restatement R comes to a select's edge: the smallest of |d - lb|, |d - ub| over the delayed commands and of
    ||l - a_prev| - du| over the knots, per sample [S].  A select cannot flip on rounding where this is far above the parity
    tolerance."""
    S, N, m = R["us"].shape
    lb, ub, beta, du = _rows(m, lb, ub, beta, du)
    near = np.full(S, np.inf)
    for s in range(S):
        for i in range(N):
            d = R["ud"][s, i]
            a_prev = R["a0"] if i == 0 else R["us"][s, i - 1]
            sv = clamp(d, lb, ub)
            l = sv - beta * (sv - a_prev)
            with np.errstate(invalid="ignore"):
                cand = np.r_[np.abs(d - lb), np.abs(d - ub), np.abs(np.abs(l - a_prev) - du)]
            cand = cand[np.isfinite(cand)]
            if cand.size:
                near[s] = min(near[s], cand.min())
    return near


def actuator_state_host(u0, delay):
    """The actuator at rest on u0 [m]: [1 + delay, m], row 0 the last applied input, rows 1.. the pending commands."""
    return np.repeat(np.asarray(u0, float)[None], 1 + delay, axis=0)


def restate_mpc_step_actuated(op, q0, xi0, u0, state, lb=None, ub=None, beta=None, du=None, w=None, op_plant=None):
    """One receding-horizon step of one trajectory behind the actuator: the command c = u0 (the step's u*_0), state
    [1 + delay, m] as tolg_mpc_advance_actuated keeps it.  Returns (x_next_q, x_next_xi, applied, stage cost, the next state,
    n_sat, n_rate); `state` is left alone."""
    m = u0.shape[0]
    lb, ub, beta, du = _rows(m, lb, ub, beta, du)
    st = np.array(state, float)
    delay = st.shape[0] - 1
    d = st[1] if delay > 0 else np.asarray(u0, float)
    a, mv = actuate(d, st[0], lb, ub, beta, du)
    n_sat = int(((d < lb) | (d > ub)).sum())
    if delay > 0:
        st[1:delay] = st[2:delay + 1].copy()
        st[delay] = u0
    st[0] = a
    q1, x1 = ob.f(op if op_plant is None else op_plant, q0, xi0, a)
    if w is not None:
        x1 = x1 + w
    return q1, x1, a, ob.cost(op, q0, xi0, a, 0)[0], st, n_sat, int(mv.sum())
