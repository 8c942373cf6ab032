"""Keep-out spheres (tolg_set_al_obstacles, tolg_al_update_state): the augmented-Lagrangian terms of a state constraint added by
the cost-evaluating kernels (PT_OBS).

- zero multipliers give the bits of the solve without spheres (the terms are exact zeros added after the tracking values);
- the linearisation's l, l_x and l_xx move by exactly a NumPy restatement of the terms, on every model and PT combination;
- fixed multipliers: the GPU solve against the mirror's host generic path (oracle per-knot functions + host AL formulas);
- the outer update against a NumPy restatement of _al_update_param, alone and beside the input box;
- batch independence, argument errors, the held policy, and the full sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, _capi, workloads
from tests.checks import host_solve, update_restated
from tests.support import dense_fixed_block

pytestmark = pytest.mark.gpu
f64 = dict(dtype=torch.float64, device="cuda:0")


def _mults(B, N, K, seed, lam=1.0, imu=20.0):
    rng = np.random.default_rng(seed)
    return (torch.as_tensor(rng.uniform(0.0, lam, (B, N + 1, K)), **f64).contiguous(),
            torch.as_tensor(rng.uniform(0.0, imu, (B, N + 1, K)), **f64).contiguous())


def _terms(xs_q, obs, lam, imu):
    """NumPy restatement: per (b, i) the l, l_x[3:6] and l_xx[3:6, 3:6] the spheres add"""
    R, t = xs_q[..., :3, :3], xs_q[..., :3, 3]
    d = t[:, :, None, :] - obs[:, None, :, :3]                    # [B, N+1, K, 3]
    g = obs[:, None, :, 3] ** 2 - np.sum(d * d, axis=-1)           # [B, N+1, K]
    gv = -2.0 * np.einsum("biac,bika->bikc", R, d)                 # -2 R^T (t - c)
    l = np.sum(lam * g + 0.5 * imu * g * g, axis=-1)
    lx = np.einsum("bikc,bik->bic", gv, lam + imu * g)
    lxx = np.einsum("bik,bika,bikc->biac", imu, gv, gv)
    return g, l, lx, lxx


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


def _model(name, B, N):
    if name == "drone":
        prob, q, xi, us, obs = workloads.drone_obstacle_field(B, 3, N=N)
    else:
        prob, q, xi, us, obs = workloads.se3_obstacle_field(B, 3, N=N)
        if name == "rigidbody":
            prob = TrackingProblem("rigidbody", prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
        elif name == "dense":
            prob = dense_fixed_block(prob)
    return prob, q, xi, us, obs


MODES = [dict(mode="ms", n_iterations=10, tol_grad_norm=0.0, tol_d_norm=0.0),
         dict(mode="ms", n_iterations=10, tol_grad_norm=0.0, tol_d_norm=0.0, schedule="split"),
         dict(mode="ms", n_iterations=15, line_search=True),
         dict(mode="ss", n_iterations=15),
         dict(mode="ms", n_iterations=15, line_search=True, rollout="linear")]


@pytest.mark.parametrize("kw", MODES)
@pytest.mark.parametrize("name", ["se3", "drone"])
def test_zero_multipliers_change_nothing(name, kw):
    B, N = 6, 60 if name == "se3" else 120
    prob, q, xi, us, obs = _model(name, B, N)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.fit_batch(q, xi, us, **kw)
    z = torch.zeros(B, N + 1, obs.shape[1], **f64)
    s.set_al_obstacles(obs, z, z.clone())
    r1 = s.fit_batch(q, xi, us, **kw)
    s.set_al_obstacles(None)
    for f in ("xs_q", "xs_xi", "us", "J_hist", "iters", "status"):
        a, b = getattr(r0, f), getattr(r1, f)
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)), f


@pytest.mark.parametrize("pt", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", ["se3", "rigidbody", "drone", "dense"])
def test_linearisation_terms(name, pt):
    B, N = 5, 30
    prob, q, xi, us, obs = _model(name, B, N)
    rng = np.random.default_rng(3)
    xs_q = np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy()
    xs_q[..., :3, 3] += 0.05 * rng.normal(size=(B, N + 1, 3))
    xs_xi = np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape) + 0.1 * rng.normal(size=(B, N + 1, 6))
    us = 0.1 * rng.normal(size=(B, N, prob.m))
    kw = {}
    if pt[0]:
        kw.update(q_ref=xs_q + 0.0, xi_ref=xs_xi * 0.9)
        kw["q_ref"][..., :3, 3] += 0.02
    if pt[1]:
        d = np.exp(rng.uniform(-0.5, 0.5, (B, 12 + 12 + prob.m)))
        kw.update(Q=d[:, :12, None] * np.eye(12) * np.diag(prob.Q)[:, None], P=d[:, 12:24, None] * np.eye(12) * np.diag(prob.P)[:, None],
                  R=d[:, 24:, None] * np.eye(prob.m) * np.diag(prob.R)[:, None])
    s = BatchedTrackingILQR(prob, B)
    a = s.linearize_backward(xs_q, xs_xi, us, **kw)
    lam, imu = _mults(B, N, obs.shape[1], 5)
    s.set_al_obstacles(obs, lam, imu)
    b = s.linearize_backward(xs_q, xs_xi, us, **kw)
    s.set_al_obstacles(None)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    g, l, lx, lxx = _terms(xs_q, obs, host(lam), host(imu))
    assert (g > 0).any()  # active spheres
    assert _close(host(b["J"]) - host(a["J"]), l.sum(axis=1))
    assert _close(host(b["lx"])[..., 3:6] - host(a["lx"])[..., 3:6], lx)
    assert torch.equal(b["lx"][..., :3], a["lx"][..., :3]) and torch.equal(b["lx"][..., 6:], a["lx"][..., 6:])
    assert _close(host(b["lxx11"])[..., 3:, 3:] - host(a["lxx11"])[..., 3:, 3:], lxx)
    assert torch.equal(b["lxx11"][..., :3, :], a["lxx11"][..., :3, :]) and torch.equal(b["lxx11"][..., 3:, :3], a["lxx11"][..., 3:, :3])


@pytest.mark.parametrize("kw", [dict(mode="ms", n_iterations=6), dict(mode="ms", n_iterations=6, line_search=True),
                                dict(mode="ss", n_iterations=6), dict(mode="ms", n_iterations=6, rollout="linear")])
def test_fixed_multiplier_parity_with_the_host_generic_path(kw):
    B, N = 3, 40
    obs = workloads.se3_obstacle_field(B, 2, N=N, seed=11)[4]
    prob, q, xi, us0 = workloads.se3_tracking(B, N=N, R_scale=1e-3)
    lam, imu = _mults(B, N, 2, 9, lam=0.5, imu=5.0)
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu)
    r = s.fit_batch(q, xi, us0, tol_grad_norm=0.0, tol_d_norm=0.0, check_every=0, **kw)
    s.set_al_obstacles(None)
    for b in range(B):
        J, us = host_solve(prob, q[b], xi[b], us0[b], obs[b], lam[b].cpu().numpy(), imu[b].cpu().numpy(), kw)
        n = int(r.iters[b])
        assert n == len(J) and int(r.status[b]) == 0
        assert np.abs(r.J_hist[b, :n].cpu().numpy() / J - 1).max() < 1e-9
        ug = r.us[b].cpu().numpy()
        assert np.abs(ug - us).max() < 1e-6 * max(1.0, np.abs(us).max())


@pytest.mark.parametrize("box", [False, True])
def test_outer_update_against_a_restatement(box):
    B, N = 2, 40
    prob, q, xi, us0, obs = workloads.se3_obstacle_field(B, 3, N=N)
    s = BatchedTrackingILQR(prob, B)
    kw = dict(lb=-3.0 * np.ones(6), ub=3.0 * np.ones(6)) if box else {}
    res, info = s.al_fit_batch(q, xi, us0, n_al_iters=1, n_ilqr_iters=30, obstacles=obs, mu0=1e-2, **kw)
    xs_q = res.xs_q.cpu().numpy()
    g = obs[:, None, :, 3] ** 2 - np.sum((xs_q[..., :3, 3][:, :, None] - obs[:, None, :, :3]) ** 2, axis=-1)
    ln, im = update_restated(g, 0.0, 1e-2, 1e-2)
    mv = g.max(axis=(1, 2))
    if box:
        u = res.us.cpu().numpy()
        gb = np.concatenate([kw["lb"] - u, u - kw["ub"]], axis=-1)
        mv = np.maximum(mv, np.maximum(gb.max(axis=(1, 2)), 0.0))
        lb_, ib_ = update_restated(gb, 0.0, 1e-2, 1e-2)
        assert np.array_equal(info["lmbd"].cpu().numpy(), lb_) and np.array_equal(info["Imu"].cpu().numpy(), ib_)
    assert np.all(mv > 1e-2)  # the first solve violates
    assert np.allclose(info["max_violation"].cpu().numpy(), mv, rtol=1e-12, atol=0)
    assert np.allclose(info["lmbd_obs"].cpu().numpy(), ln, rtol=1e-12, atol=1e-15)
    assert np.array_equal(info["Imu_obs"].cpu().numpy(), im)
    assert np.allclose(info["mu"].cpu().numpy(), 1e-1)


@pytest.mark.parametrize("box", [False, True])
def test_outer_loop(box):
    """The whole outer loop: the first solve violates; a problem marked converged keeps every constraint within tol_constr (the
    spheres on its final states, the box on its final controls)"""
    B, N = 2, 40
    prob, q, xi, us0, obs = workloads.se3_obstacle_field(B, 3, N=N)
    s = BatchedTrackingILQR(prob, B)
    kw = dict(lb=-10.0 * np.ones(6), ub=10.0 * np.ones(6)) if box else {}
    tol = 1e-2
    first = []
    res, info = s.al_fit_batch(q, xi, us0, n_al_iters=20, n_ilqr_iters=100, obstacles=obs, tol_constr=tol, line_search=True,
                               on_outer=lambda it, r, *a: first.append(r.xs_q.clone()) if it == 0 else None, **kw)
    assert info["outer_iterations"] > 1
    xs_q = res.xs_q.cpu().numpy()
    gmax = lambda x: (obs[:, None, :, 3] ** 2 - np.sum((x[..., :3, 3][:, :, None] - obs[:, None, :, :3]) ** 2, axis=-1)).max(axis=(1, 2))  # noqa: E731
    g, g0 = gmax(xs_q), gmax(first[0].cpu().numpy())
    assert np.all(g0 > tol)
    conv = info["al_converged"].cpu().numpy().astype(bool)
    assert conv.any()
    assert np.all(g[conv] < tol)
    if box:
        assert np.all(res.us.abs().amax(dim=(1, 2)).cpu().numpy()[conv] < 10.0 + tol)
    assert (info["lmbd_obs"] >= 0).all() and (info["lmbd_obs"] > 0).any()


def test_batch_independence():
    B, N = 8, 60
    prob, q, xi, us, obs = workloads.se3_obstacle_field(B, 3, N=N)
    lam, imu = _mults(B, N, 3, 2)
    kw = dict(mode="ms", n_iterations=10, line_search=True)
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu)
    r = s.fit_batch(q, xi, us, **kw)
    s.set_al_obstacles(None)
    j = 5
    rep = lambda a: np.broadcast_to(np.asarray(a)[j], (4,) + np.shape(a)[1:]).copy()  # noqa: E731
    s4 = BatchedTrackingILQR(prob, 4)
    s4.set_al_obstacles(rep(obs), lam[j:j + 1].repeat(4, 1, 1).contiguous(), imu[j:j + 1].repeat(4, 1, 1).contiguous())
    r4 = s4.fit_batch(rep(q), rep(xi), rep(us), **kw)
    s4.set_al_obstacles(None)
    a, b = r.us[j].cpu().numpy(), r4.us[0].cpu().numpy()
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert int(r.iters[j]) == int(r4.iters[0])


def test_argument_errors_and_the_held_policy():
    B, N = 3, 20
    prob, q, xi, us, obs = workloads.se3_obstacle_field(B, 2, N=N)
    s = BatchedTrackingILQR(prob, 4)
    lib, h = s.lib, s._h
    lam, imu = _mults(B, N, 2, 1)
    d = torch.as_tensor(obs, **f64).contiguous()
    buf = torch.empty(lib.tolg_obstacles_bytes(C.byref(s._p), 4, 16) // 8, **f64)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nb = C.c_size_t(buf.numel() * 8)
    st = s._stream()
    assert lib.tolg_set_al_obstacles(h, 0, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert lib.tolg_set_al_obstacles(h, 5, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert lib.tolg_set_al_obstacles(h, B, 0, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert lib.tolg_set_al_obstacles(h, B, 17, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert lib.tolg_set_al_obstacles(h, B, 2, P(d), P(lam), P(imu), P(buf), C.c_size_t(8), st) == -1
    assert lib.tolg_set_al_obstacles(h, B, 2, P(d), None, P(imu), P(buf), nb, st) == -1
    assert lib.tolg_al_update_state(h, B, None, None, P(lam), 10.0, 1e8, 1e-2, P(lam), P(lam), st) == -1  # nothing attached
    # references per trajectory for another B
    s.fit_batch(q[:2], xi[:2], us[:2], n_iterations=2, q_ref=np.broadcast_to(prob.q_ref, (2,) + prob.q_ref.shape),
                xi_ref=np.broadcast_to(prob.xi_ref, (2,) + prob.xi_ref.shape))
    assert lib.tolg_set_al_obstacles(h, B, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    s.clear_per_trajectory()
    # a solve in flight
    s.solve_begin(q, xi, us, n_iterations=2)
    assert lib.tolg_set_al_obstacles(h, B, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    s.solve_iterate(2)
    s.solve_end()
    K0 = s.gains()["K"]  # the held policy survives attaching the spheres
    s.set_al_obstacles(obs, lam, imu)
    assert torch.equal(s.gains()["K"], K0)
    with pytest.raises(RuntimeError):  # batch calls for another B
        s.fit_batch(q[:2], xi[:2], us[:2], n_iterations=2)
    s.set_al_obstacles(None)
    for bad in (np.zeros((B, 2, 3)), np.concatenate([obs[..., :3], -np.ones((B, 2, 1))], -1), np.full((B, 17, 4), 1.0),
                np.full((B, 2, 4), np.nan)):
        with pytest.raises(ValueError):
            s.set_al_obstacles(bad, lam, imu)
    so3 = workloads.so3_tracking(2, N=20)[0]
    s3 = BatchedTrackingILQR(so3, 2)
    with pytest.raises(ValueError):
        s3.set_al_obstacles(np.array([[0, 0, 0, 1.0]]), torch.zeros(2, 21, 1, **f64), torch.zeros(2, 21, 1, **f64))
    buf3 = torch.empty(64, **f64)
    assert s3.lib.tolg_set_al_obstacles(s3._h, 2, 1, P(d), P(lam), P(imu), P(buf3), C.c_size_t(512), st) == -1


@pytest.mark.parametrize("name, B, N, tol", [("se3", 4096, 200, 1e-2), ("drone", 1024, 400, 1e-3)])
def test_full_size(name, B, N, tol):
    f = workloads.se3_obstacle_field if name == "se3" else workloads.drone_obstacle_field
    prob, q, xi, us, obs = f(B, 8, N=N)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.fit_batch(q, xi, us, n_iterations=100, line_search=True)
    gmax = lambda x: (obs[:, None, :, 3] ** 2 - np.sum((x[..., :3, 3][:, :, None] - obs[:, None, :, :3]) ** 2, axis=-1)).max(axis=(1, 2))  # noqa: E731
    g0 = gmax(r0.xs_q.cpu().numpy())
    assert np.mean(g0 > tol) > 0.5  # the unconstrained solve violates
    res, info = s.al_fit_batch(q, xi, us, n_al_iters=10, n_ilqr_iters=100, obstacles=obs, tol_constr=tol, line_search=True)
    for t in (res.xs_q, res.us, info["lmbd_obs"], info["max_violation"]):
        assert torch.isfinite(t).all()
    assert not (res.status == _capi.ST_INTERNAL).any()
    conv = info["al_converged"].cpu().numpy().astype(bool)
    g = gmax(res.xs_q.cpu().numpy())
    assert conv.any() and np.all(g[conv] < tol)
    # the batch as a whole moves out of the spheres (the drone at tol 1e-3 does not finish in 10 outer iterations: DESIGN.md)
    assert np.median(g) < 0.5 * np.median(g0)
