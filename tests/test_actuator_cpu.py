"""The actuator model of the actuated closed loops, without a GPU: the host restatement of tests/actuator.py against
tests/limits.py and against the closed forms of its pieces (pure delay, pure lag, rate limit), the one-step form with its state
array against the rollout form, and check_actuator's conversions and refusals."""
import numpy as np
import pytest

from trajectory_optimization_matrix_lie_groups_amd import actuator_state, check_actuator, workloads
from tests.actuator import actuate, actuator_state_host, edge_distance, restate_mpc_step_actuated, restate_policy_actuated
from tests.estimated import open_loop_policy
from tests.limits import clamp, restate_policy_limited
from tests.support import pert

N, S = 12, 4


@pytest.fixture(scope="module")
def policy():
    prob, q, xi, us = workloads.se3_tracking(1, N=N, R_scale=1e-3)
    op, qn, xn, un, K = open_loop_policy(prob, q[0], xi[0], us[0])
    dx0, w = pert(1, S, N, seed=11)
    return op, qn, xn, un, K, dx0[0], w[0]


def _box(un, frac=0.5):
    lo, hi = un.min(axis=0), un.max(axis=0)
    return lo + frac * 0.25 * (hi - lo), hi - frac * 0.25 * (hi - lo)


def test_neutral_model_is_the_limited_restatement(policy):
    op, qn, xn, un, K, dx0, w = policy
    lb, ub = _box(un)
    L = restate_policy_limited(op, qn, xn, un, K, lb, ub, dx0, w, S)
    assert L["n_sat"].sum() > 0
    for kw in (dict(), dict(beta=np.zeros(6), du=np.full(6, np.inf), delay=0, u_init=np.full(6, 7.0))):
        A = restate_policy_actuated(op, qn, xn, un, K, lb, ub, dx0=dx0, noise=w, S=S, **kw)
        for k in ("J", "xs_q", "xs_xi", "us", "uc", "n_sat", "u_excess"):
            assert np.array_equal(A[k], L[k]), k
        assert (A["n_rate"] == 0).all() and np.array_equal(A["ud"], A["uc"])
        assert np.array_equal(A["u_gap"], np.abs(L["us"] - L["uc"]).max(axis=(1, 2)))


@pytest.mark.parametrize("D", [1, 4])
def test_pure_delay(policy, D):
    op, qn, xn, un, K, dx0, w = policy
    lb, ub = _box(un)
    u_init = un[0] + 0.1
    A = restate_policy_actuated(op, qn, xn, un, K, lb, ub, delay=D, u_init=u_init, dx0=dx0, noise=w, S=S)
    assert np.array_equal(A["us"][:, D:], clamp(A["uc"][:, :-D], lb, ub))
    assert np.array_equal(A["us"][:, :D], np.broadcast_to(clamp(u_init, lb, ub), (S, D, 6)))
    assert (A["n_rate"] == 0).all()


def test_delay_beyond_the_horizon_applies_u_init_alone(policy):
    op, qn, xn, un, K, dx0, w = policy
    A = restate_policy_actuated(op, qn[:4], xn[:4], un[:3], K[:3], delay=4, u_init=un[0], dx0=dx0, noise=w[:, :3], S=S)
    assert np.array_equal(A["us"], np.broadcast_to(un[0], (S, 3, 6)))
    B = restate_policy_actuated(op, qn[:4], xn[:4], un[:3], K[:3], delay=4, dx0=dx0, noise=w[:, :3], S=S)
    assert all(np.array_equal(A[k], B[k]) for k in ("J", "us", "xs_q", "xs_xi", "u_gap"))


def test_pure_lag_follows_one_minus_beta_to_the_k():
    beta = np.array([0.0, 0.3, 0.9])
    c, a = np.array([1.0, -2.0, 0.5]), np.zeros(3)
    for k in range(1, 30):
        a, mv = actuate(c, a, -np.inf, np.inf, beta, np.inf)
        assert not mv.any()
        assert np.abs(a - c * (1.0 - beta ** k)).max() < 1e-14
    assert a[0] == c[0]  # beta = 0: the command itself, from the first knot


def test_rate_limit_bounds_every_step_and_counts_the_bound_ones(policy):
    op, qn, xn, un, K, dx0, w = policy
    free = restate_policy_actuated(op, qn, xn, un, K, dx0=dx0, noise=w, S=S)
    steps = np.abs(np.diff(np.concatenate([np.broadcast_to(un[0], (S, 1, 6)), free["us"]], axis=1), axis=1))
    du = np.median(steps, axis=(0, 1))  # about half of the free loop's steps are larger
    A = restate_policy_actuated(op, qn, xn, un, K, du=du, dx0=dx0, noise=w, S=S)
    a = np.concatenate([np.broadcast_to(un[0], (S, 1, 6)), A["us"]], axis=1)
    d = np.abs(np.diff(a, axis=1))
    assert (d <= du + 1e-12).all()  # (a + du) - a is du up to the rounding of the sum
    assert A["n_rate"].sum() > 0 and (~A["moved"]).sum() > 0
    # a bound step moves by du exactly (up to the rounding of a + du - a); a free one reaches the command
    assert np.abs(d[A["moved"]] - np.broadcast_to(du, d.shape)[A["moved"]]).max() < 1e-12
    assert np.array_equal(A["us"][~A["moved"]], A["uc"][~A["moved"]])
    assert np.array_equal(A["n_rate"], A["moved"].sum(axis=(1, 2)))
    assert np.isfinite(edge_distance(A, du=du)).all()


@pytest.mark.parametrize("D", [0, 2])
def test_one_step_form_with_its_state_array_is_the_rollout_form(policy, D):
    """Driven with the rollout's own commands and states, the MPC step reproduces the rollout's applied inputs knot by knot."""
    op, qn, xn, un, K, dx0, w = policy
    lb, ub = _box(un)
    beta, du = np.full(6, 0.4), np.full(6, 0.5)
    A = restate_policy_actuated(op, qn, xn, un, K, lb, ub, beta, du, D, dx0=dx0, noise=w, S=1)
    st = actuator_state_host(un[0], D)
    assert st.shape == (1 + D, 6)
    ns = nr = 0
    for i in range(N):
        keep = st.copy()
        q1, x1, a, _, st2, n_sat, n_rate = restate_mpc_step_actuated(op, A["xs_q"][0, i], A["xs_xi"][0, i], A["uc"][0, i], st,
                                                                     lb, ub, beta, du, w=w[0, i])
        assert np.array_equal(st, keep)  # the caller's state is left alone
        assert np.array_equal(a, A["us"][0, i]) and np.array_equal(st2[0], a)
        assert np.array_equal(q1, A["xs_q"][0, i + 1]) and np.array_equal(x1, A["xs_xi"][0, i + 1])
        if D:
            assert np.array_equal(st2[D], A["uc"][0, i]) and np.array_equal(st2[1:D], st[2:])
        st, ns, nr = st2, ns + n_sat, nr + n_rate
    assert ns == A["n_sat"][0] and nr == A["n_rate"][0]


def test_check_actuator_converts():
    dt = 0.05
    lb, ub, beta, du, ui, D = check_actuator([-1.0] * 6, [1.0] * 6, [0.0, 0.05, 0.1, 0.0, 1.0, 1e-9], 2.0, 3, np.zeros(6), 2, 6, dt)
    assert lb.shape == ub.shape == beta.shape == du.shape == ui.shape == (2, 6) and D == 3
    assert beta[0, 0] == 0.0 and beta[0, 3] == 0.0 and beta[0, 5] == 0.0  # tau = 0 (and a tau far below dt): no lag, exactly
    assert np.array_equal(beta[0, [1, 2, 4]], np.exp(-dt / np.array([0.05, 0.1, 1.0])))
    assert (beta >= 0).all() and (beta < 1).all()
    assert np.array_equal(du, np.full((2, 6), 2.0 * dt))
    none = check_actuator(None, None, None, None, 0, None, 2, 6, dt)
    assert none == (None, None, None, None, None, 0)
    assert np.isinf(check_actuator(None, None, None, np.inf, 0, None, 2, 6, dt)[3]).all()
    per_traj = check_actuator(None, None, np.array([[0.1] * 4, [0.0] * 4]), None, np.int64(1), None, 2, 4, dt)
    assert (per_traj[2][1] == 0.0).all() and (per_traj[2][0] > 0).all() and per_traj[5] == 1


@pytest.mark.parametrize("kw", [
    dict(delay=5), dict(delay=-1), dict(delay=1.0), dict(delay=True), dict(delay=None),
    dict(tau=-0.1), dict(tau=np.inf), dict(tau=np.nan), dict(tau=[0.1] * 5), dict(tau=np.zeros((3, 6))),
    dict(rate=0.0), dict(rate=-1.0), dict(rate=np.nan), dict(rate=[1.0] * 7),
    dict(u_init=np.inf), dict(u_init=[0.0] * 5), dict(u_init=np.nan),
    dict(u_lb=[-1.0] * 6), dict(u_ub=[1.0] * 6), dict(u_lb=[1.0] * 6, u_ub=[-1.0] * 6), dict(dt=0.0), dict(dt=-1.0),
])
def test_check_actuator_refuses(kw):
    a = dict(u_lb=None, u_ub=None, tau=None, rate=None, delay=0, u_init=None, B=2, m=6, dt=0.05)
    a.update(kw)
    if np.ndim(a["tau"]) == 0 and a["tau"] is not None:
        a["tau"] = np.full(6, a["tau"])
    if np.ndim(a["rate"]) == 0 and a["rate"] is not None:
        a["rate"] = np.full(6, a["rate"])
    if np.ndim(a["u_init"]) == 0 and a["u_init"] is not None:
        a["u_init"] = np.full(6, a["u_init"])
    with pytest.raises(ValueError):
        check_actuator(**a)


def test_check_actuator_so3_rows():
    dt = 0.02
    lb, ub, beta, du, ui, _ = check_actuator([-1.0] * 3, [1.0] * 3, [0.1] * 3, [2.0] * 3, 0, [0.1] * 3, 2, 6, dt, so3=True)
    assert np.isneginf(lb[:, 3:]).all() and np.isposinf(ub[:, 3:]).all()
    assert (beta[:, 3:] == 0.0).all() and np.isposinf(du[:, 3:]).all() and (ui[:, 3:] == 0.0).all()
    with pytest.raises(ValueError):  # the box rows 3..5 must contain 0
        check_actuator([-1.0] * 3 + [0.5] * 3, [1.0] * 6, None, None, 0, None, 2, 6, dt, so3=True)
    with pytest.raises(ValueError):  # u_init rows 3..5 must be 0
        check_actuator(None, None, None, None, 0, [0.0] * 3 + [0.1] * 3, 2, 6, dt, so3=True)
    with pytest.raises(ValueError):  # [3] rows are the SO3 family's alone
        check_actuator(None, None, [0.1] * 3, None, 0, None, 2, 6, dt)


def test_actuator_state_helper():
    u0 = np.arange(8.0).reshape(2, 4)
    st = actuator_state(u0, 2)
    assert st.shape == (2, 3, 4) and all(np.array_equal(st[:, k], u0) for k in range(3))
    assert np.array_equal(actuator_state(u0, 0), u0[:, None])
    assert np.array_equal(st[0], actuator_state_host(u0[0], 2))
    for bad in (5, -1, 1.5, True):
        with pytest.raises(ValueError):
            actuator_state(u0, bad)
    with pytest.raises(ValueError):
        actuator_state(u0[0], 1)


def test_workloads_are_consistent():
    prob, q, xi, us, dx0, w, act = workloads.drone_actuated(3, 5, N=20)
    assert dx0.shape == (3, 5, 12) and w.shape == (3, 5, 20, 6) and us.shape == (3, 20, 4)
    check_actuator(None, None, act["act_tau"], act["act_rate"], act["act_delay"], None, 3, 4, prob.dt)
    prob, q, xi, us, Q, P, R, gain, high, dx0, w, act = workloads.se3_gain_sweep_actuated(8, 4, N=20)
    assert Q.shape == (8, 12, 12) and R.shape == (8, 6, 6) and high.sum() == 4 and (np.diff(gain) > 0).all()
    assert (gain[high].min() > gain[~high].max()) and np.allclose(Q[:, 0, 0] * R[:, 0, 0], prob.Q[0, 0] * prob.R[0, 0])
    assert all(np.array_equal(q[b], q[0]) for b in range(8))
    check_actuator(None, None, act["act_tau"], None, act["act_delay"], None, 8, 6, prob.dt)
