"""Helpers of the moving keep-out sphere tests (tests/test_moving_obstacles_cpu.py, tests/test_gpu_moving_obstacles.py): the
per-knot restatement of the spheres' terms, the mirror's host generic path on a per-knot field, and prioritised fleet planning
on that path.  A plain module (pytest does not collect it)."""
import warnings

import numpy as np

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_constraints import MovingSphereObstacleConstraint
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_controller import (iLQR_Tracking_SE3,
                                                                                           iLQR_Tracking_SE3_MS)
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_cost import ALConstrainedCost
from tests.restate import MyCost, MyDynamics


def g_per_knot(xs_q, obs):
    """g [B, N+1, K] of positions xs_q [B, N+1, 4, 4] against a per-knot field obs [B, N+1, K, 4]"""
    d = xs_q[..., :3, 3][:, :, None, :] - obs[..., :3]
    return obs[..., 3] ** 2 - np.sum(d * d, axis=-1)


def terms_per_knot(xs_q, obs, lam, imu):
    """_terms of tests/test_gpu_obstacles.py with the geometry of every knot its own: per (b, i) the l, l_x[3:6] and
    l_xx[3:6, 3:6] the spheres obs [B, N+1, K, 4] add"""
    R, t = xs_q[..., :3, :3], xs_q[..., :3, 3]
    d = t[:, :, None, :] - obs[..., :3]                            # [B, N+1, K, 3]
    g = obs[..., 3] ** 2 - np.sum(d * d, axis=-1)                  # [B, N+1, K]
    gv = -2.0 * np.einsum("biac,bika->bikc", R, d)                 # -2 R^T (t - c)
    l = np.sum(lam * g + 0.5 * imu * g * g, axis=-1)
    lx = np.einsum("bikc,bik->bic", gv, lam + imu * g)
    lxx = np.einsum("bik,bika,bikc->biac", imu, gv, gv)
    return g, l, lx, lxx


def host_solve_moving(prob, x0_q, x0_xi, us0, obs, lam, imu, kw, q_ref=None, xi_ref=None):
    """host_solve of tests/checks.py on a per-knot field obs [N+1, K, 4]: the mirror's host generic path with fixed
    multipliers lam, imu [N+1, K].  kw: mode, n_iterations, line_search, rollout, and optionally tol_grad_norm / tol_d_norm
    (0 otherwise).  Returns (J per iteration, us, positions [N+1, 3])."""
    q_ref = prob.q_ref if q_ref is None else q_ref
    xi_ref = prob.xi_ref if xi_ref is None else xi_ref
    op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, q_ref, xi_ref)
    c = MovingSphereObstacleConstraint(obs[..., :3], obs[..., 3])
    al = ALConstrainedCost(MyCost(op, prob.m), c, prob.N)
    al.lmbd = lam.copy()
    al.Imu = np.stack([np.diag(d) for d in imu])
    ms = kw["mode"] == "ms"
    J = []

    def cb(*a):
        a[-5 if ms else -3].append(a[3])
        J.append(a[3])

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rollout = kw.get("rollout", "nonlinear")
        if ms:
            ctl = iLQR_Tracking_SE3_MS(MyDynamics(op, prob.m), al, prob.N, q_ref, xi_ref, rollout=rollout,
                                       line_search=kw.get("line_search", False))
            tol = dict(tol_grad_norm=kw.get("tol_grad_norm", 0.0), tol_d_norm=kw.get("tol_d_norm", 0.0))
        else:
            ctl = iLQR_Tracking_SE3(MyDynamics(op, prob.m), al, prob.N, rollout=rollout)
            tol = dict(tol_grad_norm=kw.get("tol_grad_norm", 0.0))
        xs, us, *_ = ctl.fit([x0_q, x0_xi], us0, n_iterations=kw["n_iterations"], on_iteration=cb, **tol)
    return np.array(J), us, np.stack([np.asarray(x[0])[:3, 3] for x in xs])


def host_member(prob, x0_q, x0_xi, q_ref, xi_ref, others, separation, n_al=12, n_ilqr=30, tol=1e-3, mu0=1e-2, mu_scale=10.0,
                mu_max=1e8):
    """One round of prioritised planning on the host path: the member tracking (q_ref, xi_ref) from (x0_q, x0_xi) keeps
    `separation` from the positions others [p, N+1, 3] at every knot; the outer rule of al_fit_batch (every outer iteration
    re-solves from the start and zero inputs, n_ilqr MS iterations with its inner tolerances 1e-6).  Returns (the
    unconstrained positions, the final positions, outer iterations used or None when max g >= tol after n_al of them)."""
    N = prob.N
    K = max(1, len(others))
    obs = np.empty((N + 1, K, 4))
    obs[..., 3] = separation
    obs[..., :3] = np.moveaxis(np.asarray(others), 0, 1) if len(others) else 1e3  # (no other member: one sphere far away)
    kw = dict(mode="ms", n_iterations=n_ilqr, tol_grad_norm=1e-6, tol_d_norm=1e-6)
    us0 = np.zeros((N, prob.m))
    zero = np.zeros((N + 1, K))
    free = host_solve_moving(prob, x0_q, x0_xi, us0, obs, zero, zero, kw, q_ref, xi_ref)[2]
    if not len(others):
        return free, free, 1
    lam, imu, mu = zero.copy(), np.full((N + 1, K), mu0), mu0
    t = free
    for outer in range(n_al):
        t = host_solve_moving(prob, x0_q, x0_xi, us0, obs, lam, imu, kw, q_ref, xi_ref)[2]
        g = obs[..., 3] ** 2 - np.sum((t[:, None, :] - obs[..., :3]) ** 2, axis=-1)
        if g.max() < tol:
            return free, t, outer + 1
        mu = min(mu * mu_scale, mu_max)  # (tolg_al_update_state's rule, as update_restated of tests/checks.py states it)
        lam = np.maximum(0.0, lam + imu * g)
        imu = np.where((g < 0) & (lam == 0), 0.0, mu)
    return free, t, None


def host_fleet(prob, x0_q, x0_xi, q_ref, xi_ref, separation, **kw):
    """Prioritised planning of one fleet (members in priority order) on the host path.  Returns (the smallest centre distance
    of the unconstrained plans over knots and pairs, of the final plans, the outer iterations of every member)."""
    free, plan, outers = [], [], []
    for p in range(len(x0_q)):
        f, t, n = host_member(prob, x0_q[p], x0_xi[p], q_ref[p], xi_ref[p], plan, separation, **kw)
        free.append(f); plan.append(t); outers.append(n)
    sep = lambda ts: min(np.linalg.norm(ts[a] - ts[b], axis=-1).min() for a in range(len(ts)) for b in range(a))  # noqa: E731
    return sep(free), sep(plan), outers
