"""Keep-out spheres that move (tolg_set_al_obstacles_moving): the geometry of every knot its own, through the kernels of the
static form with a knot stride.

- a field that is constant in time gives the bits of the static form, in every solve path and in al_fit_batch;
- the linearisation's l, l_x and l_xx move by a NumPy restatement of the per-knot terms, on every model and PT combination;
- fixed multipliers: the GPU solve against the mirror's host generic path with MovingSphereObstacleConstraint;
- the outer update against a restatement with per-knot g, both forms, detach and re-attach, argument errors;
- batch independence;
- plan_fleet: prioritised deconfliction of crossing fleets."""
import ctypes as C

import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, workloads
from tests.checks import update_restated
from tests.moving import g_per_knot, host_solve_moving, terms_per_knot
from tests.support import assert_bitwise, bits, dense_fixed_block

pytestmark = pytest.mark.gpu
f64 = dict(dtype=torch.float64, device="cuda:0")


def _mults(B, N, K, seed, lam=1.0, imu=20.0):
    rng = np.random.default_rng(seed)
    return (torch.as_tensor(rng.uniform(0.0, lam, (B, N + 1, K)), **f64).contiguous(),
            torch.as_tensor(rng.uniform(0.0, imu, (B, N + 1, K)), **f64).contiguous())


def _close(a, b, rel=1e-12):  # the tolerance of test_linearisation_terms (tests/test_gpu_obstacles.py)
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


def _model(name, B, N, K):
    if name == "drone":
        prob, q, xi, us, obs = workloads.drone_obstacle_field(B, K, N=N)
    else:
        prob, q, xi, us, obs = workloads.se3_obstacle_field(B, K, N=N)
        if name == "rigidbody":
            prob = TrackingProblem("rigidbody", prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
        elif name == "dense":
            prob = dense_fixed_block(prob)
    return prob, q, xi, us, obs


def _repeat(obs, N):
    return np.ascontiguousarray(np.broadcast_to(obs[:, None], (obs.shape[0], N + 1) + obs.shape[1:]))


MODES = [dict(mode="ms", n_iterations=8, tol_grad_norm=0.0, tol_d_norm=0.0),
         dict(mode="ms", n_iterations=10, line_search=True),
         dict(mode="ss", n_iterations=10),
         dict(mode="ms", n_iterations=10, line_search=True, rollout="linear")]


@pytest.mark.parametrize("kw", MODES)
@pytest.mark.parametrize("name, B, N, K", [("se3", 5, 30, 3), ("drone", 6, 40, 1)])
def test_constant_in_time_equals_static_to_the_bit(name, B, N, K, kw):
    prob, q, xi, us, obs = _model(name, B, N, K)
    lam, imu = _mults(B, N, K, 4)
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu)
    r0 = s.fit_batch(q, xi, us, **kw)
    s.set_al_obstacles(_repeat(obs, N), lam, imu)  # replaces the static form
    r1 = s.fit_batch(q, xi, us, **kw)
    s.set_al_obstacles(None)
    r2 = s.fit_batch(q, xi, us, **kw)
    assert_bitwise(r0, r1, what="moving against static")
    assert not torch.equal(bits(r0.us), bits(r2.us))  # the spheres act


def test_constant_in_time_al_fit_batch_equals_static_to_the_bit():
    B, N, K = 5, 30, 3
    prob, q, xi, us, obs = _model("se3", B, N, K)
    s = BatchedTrackingILQR(prob, B)
    kw = dict(n_al_iters=3, n_ilqr_iters=20, tol_constr=1e-3)
    r0, i0 = s.al_fit_batch(q, xi, us, obstacles=obs, **kw)
    r1, i1 = s.al_fit_batch(q, xi, us, obstacles=_repeat(obs, N), **kw)
    assert_bitwise(r0, r1, what="al_fit_batch moving against static")
    assert sorted(i0) == sorted(i1) and i0["outer_iterations"] == i1["outer_iterations"]
    for k in ("lmbd_obs", "Imu_obs", "mu", "max_violation", "al_converged"):
        assert torch.equal(bits(i0[k]), bits(i1[k])), k
    assert (i0["lmbd_obs"] > 0).any()


@pytest.mark.parametrize("pt", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name, K", [("se3", 3), ("rigidbody", 1), ("drone", 3), ("dense", 3)])
def test_per_knot_linearisation_terms(name, K, pt):
    B, N = 5, 24
    prob, q, xi, us, _ = _model(name, B, N, K)
    rng = np.random.default_rng(3)
    xs_q = np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy()
    xs_q[..., :3, 3] += 0.05 * rng.normal(size=(B, N + 1, 3))
    xs_xi = np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape) + 0.1 * rng.normal(size=(B, N + 1, 6))
    us = 0.1 * rng.normal(size=(B, N, prob.m))
    # geometry drawn independently at every knot, the radius too: near the trajectory, so that spheres are active
    obs = np.empty((B, N + 1, K, 4))
    obs[..., :3] = xs_q[..., :3, 3][:, :, None, :] + 0.3 * rng.normal(size=(B, N + 1, K, 3))
    obs[..., 3] = rng.uniform(0.2, 0.6, (B, N + 1, K))
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
    lam, imu = _mults(B, N, K, 5)
    s.set_al_obstacles(obs, lam, imu)
    b = s.linearize_backward(xs_q, xs_xi, us, **kw)
    s.set_al_obstacles(None)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    g, l, lx, lxx = terms_per_knot(xs_q, obs, host(lam), host(imu))
    assert (g > 0).any() and (g < 0).any()
    dlx = host(b["lx"])[..., 3:6] - host(a["lx"])[..., 3:6]
    dlxx = host(b["lxx11"])[..., 3:, 3:] - host(a["lxx11"])[..., 3:, 3:]
    assert _close(host(b["J"]) - host(a["J"]), l.sum(axis=1))
    assert _close(dlx, lx) and _close(dlxx, lxx)
    for i in (0, N):  # the first knot and the terminal one, each against its own geometry
        assert _close(dlx[:, i], lx[:, i]) and _close(dlxx[:, i], lxx[:, i])
        assert np.abs(lx[:, i]).min() > 0
    # ... and against no other knot's: the terms of knot 0's geometry at every knot are something else
    wrong = terms_per_knot(xs_q, _repeat(obs[:, 0], N), host(lam), host(imu))[2]
    assert not _close(dlx[:, N], wrong[:, N], rel=1e-3)
    assert torch.equal(b["lx"][..., :3], a["lx"][..., :3]) and torch.equal(b["lx"][..., 6:], a["lx"][..., 6:])
    assert torch.equal(b["lxx11"][..., :3, :], a["lxx11"][..., :3, :]) and torch.equal(b["lxx11"][..., 3:, :3], a["lxx11"][..., 3:, :3])


@pytest.mark.parametrize("kw", [dict(mode="ms", n_iterations=6), dict(mode="ms", n_iterations=6, line_search=True),
                                dict(mode="ss", n_iterations=6), dict(mode="ms", n_iterations=6, rollout="linear")])
def test_fixed_multiplier_parity_with_the_host_generic_path(kw):
    B, N = 3, 40
    obs = workloads.se3_moving_obstacle_field(B, 2, N=N, seed=11)[4]
    prob, q, xi, us0 = workloads.se3_tracking(B, N=N, R_scale=1e-3)
    lam, imu = _mults(B, N, 2, 9, lam=0.5, imu=5.0)
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu)
    r = s.fit_batch(q, xi, us0, tol_grad_norm=0.0, tol_d_norm=0.0, check_every=0, **kw)
    s.set_al_obstacles(None)
    for b in range(B):
        J, us, _ = host_solve_moving(prob, q[b], xi[b], us0[b], obs[b], lam[b].cpu().numpy(), imu[b].cpu().numpy(), kw)
        n = int(r.iters[b])
        assert n == len(J) and int(r.status[b]) == 0
        assert np.abs(r.J_hist[b, :n].cpu().numpy() / J - 1).max() < 1e-9
        ug = r.us[b].cpu().numpy()
        assert np.abs(ug - us).max() < 1e-6 * max(1.0, np.abs(us).max())


def test_outer_update_both_forms_detach_and_reattach():
    B, N, K = 5, 30, 3
    prob, q, xi, us0, obs = workloads.se3_moving_obstacle_field(B, K, N=N)
    static = workloads.se3_obstacle_field(B, K, N=N)[4]  # the field before it moves
    s = BatchedTrackingILQR(prob, B)
    xs_q = s.fit_batch(q, xi, us0, n_iterations=20).xs_q
    xh = xs_q.cpu().numpy()
    lam0, imu0 = _mults(B, N, K, 6, lam=0.2, imu=1e-2)
    mu0, tol = 1e-2, 1e-3

    def update():
        lam, imu = lam0.clone(), imu0.clone()
        mu, mv = torch.full((B,), mu0, **f64), torch.zeros(B, **f64)
        conv = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        return lam, imu, mu, mv, conv

    def check(field, lam, imu, mu, mv, conv):
        g = g_per_knot(xh, field)
        ln, im = update_restated(g, lam0.cpu().numpy(), imu0.cpu().numpy(), mu0)
        assert np.all(g.max(axis=(1, 2)) > tol) and not conv.any()
        assert np.allclose(mv.cpu().numpy(), g.max(axis=(1, 2)), rtol=1e-12, atol=0)
        assert np.allclose(lam.cpu().numpy(), ln, rtol=1e-12, atol=1e-15)
        assert np.array_equal(imu.cpu().numpy(), im)
        assert np.allclose(mu.cpu().numpy(), 10 * mu0)

    # moving, static, moving again, a detach, static again: every attach replaces what was there
    for field in (obs, static, obs, None, static):
        if field is None:
            s.set_al_obstacles(None)
            st = update()
            assert s.lib.tolg_al_update_state(s._h, B, C.c_void_p(xs_q.data_ptr()), None, C.c_void_p(st[2].data_ptr()), 10.0, 1e8,
                                              tol, C.c_void_p(st[3].data_ptr()), C.c_void_p(st[4].data_ptr()), s._stream()) == -1
            continue
        lam, imu, mu, mv, conv = update()
        s.set_al_obstacles(field, lam, imu)
        s._call("tolg_al_update_state", B, C.c_void_p(xs_q.data_ptr()), None, C.c_void_p(mu.data_ptr()), 10.0, 1e8, tol,
                C.c_void_p(mv.data_ptr()), C.c_void_p(conv.data_ptr()))
        check(field if field.ndim == 4 else _repeat(field, N), lam, imu, mu, mv, conv)
    s.set_al_obstacles(None)
    # detaching through the moving entry point
    lam, imu, *_ = update()
    s.set_al_obstacles(static, lam, imu)
    assert s.lib.tolg_set_al_obstacles_moving(s._h, 0, 0, None, None, None, None, 0, s._stream()) == 0
    s._obs = None
    r0 = s.fit_batch(q, xi, us0, n_iterations=5)
    assert torch.equal(bits(r0.us), bits(BatchedTrackingILQR(prob, B).fit_batch(q, xi, us0, n_iterations=5).us))


def test_argument_errors():
    B, N = 3, 20
    prob, q, xi, us, obs = workloads.se3_moving_obstacle_field(B, 2, N=N)
    s = BatchedTrackingILQR(prob, 4)
    lib, h = s.lib, s._h
    lam, imu = _mults(B, N, 2, 1)
    d = torch.as_tensor(obs, **f64).contiguous()
    n_static = lib.tolg_obstacles_bytes(C.byref(s._p), 4, 16)
    n_moving = lib.tolg_obstacles_moving_bytes(C.byref(s._p), 4, 16)
    assert n_moving == (N + 1) * n_static
    buf = torch.empty(n_moving // 8, **f64)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nb = C.c_size_t(buf.numel() * 8)
    st = s._stream()
    attach = lib.tolg_set_al_obstacles_moving
    assert attach(h, 0, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, 5, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, B, 0, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, B, 17, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, B, 2, P(d), P(lam), P(imu), P(buf), C.c_size_t(8), st) == -1
    # big enough for the static size only, and one double short of the moving size
    assert attach(h, B, 2, P(d), P(lam), P(imu), P(buf), C.c_size_t(lib.tolg_obstacles_bytes(C.byref(s._p), B, 2)), st) == -1
    assert attach(h, B, 2, P(d), P(lam), P(imu), P(buf), C.c_size_t(lib.tolg_obstacles_moving_bytes(C.byref(s._p), B, 2) - 8), st) == -1
    assert attach(h, B, 2, P(d), None, P(imu), P(buf), nb, st) == -1
    assert attach(h, B, 2, P(d), P(lam), None, P(buf), nb, st) == -1
    assert attach(h, B, 2, P(d), P(lam), P(imu), None, nb, st) == -1
    assert lib.tolg_al_update_state(h, B, None, None, P(lam), 10.0, 1e8, 1e-2, P(lam), P(lam), st) == -1  # nothing attached
    # references per trajectory for another B
    s.fit_batch(q[:2], xi[:2], us[:2], n_iterations=2, q_ref=np.broadcast_to(prob.q_ref, (2,) + prob.q_ref.shape),
                xi_ref=np.broadcast_to(prob.xi_ref, (2,) + prob.xi_ref.shape))
    assert attach(h, B, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    s.clear_per_trajectory()
    # a solve in flight
    s.solve_begin(q, xi, us, n_iterations=2)
    assert attach(h, B, 2, P(d), P(lam), P(imu), P(buf), nb, st) == -1
    s.solve_iterate(2)
    s.solve_end()
    K0 = s.gains()["K"]  # the held policy survives attaching the spheres
    s.set_al_obstacles(obs, lam, imu)
    assert torch.equal(s.gains()["K"], K0)
    assert s._obs_mov_buf.numel() * 8 == lib.tolg_obstacles_moving_bytes(C.byref(s._p), B, 2)  # for the B and K asked for
    with pytest.raises(RuntimeError):  # batch calls for another B
        s.fit_batch(q[:2], xi[:2], us[:2], n_iterations=2)
    with pytest.raises(ValueError, match="keep-out spheres"):
        s.mpc(q, xi, np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape), np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape), 1)
    s.set_al_obstacles(None)
    bad_r = obs.copy()
    bad_r[1, 3, 0, 3] = 0.0
    for bad in (obs[:, :N], obs[..., :3], bad_r, np.full((B, N + 1, 17, 4), 1.0), np.full((B, N + 1, 2, 4), np.nan)):
        with pytest.raises(ValueError):
            s.set_al_obstacles(bad, lam, imu)
    so3 = workloads.so3_tracking(2, N=20)[0]
    s3 = BatchedTrackingILQR(so3, 2)
    with pytest.raises(ValueError):
        s3.set_al_obstacles(np.ones((2, 21, 1, 4)), torch.zeros(2, 21, 1, **f64), torch.zeros(2, 21, 1, **f64))
    assert s3.lib.tolg_set_al_obstacles_moving(s3._h, 2, 1, P(d), P(lam), P(imu), P(buf), nb, st) == -1


def test_batch_independence():
    """A trajectory's bits do not depend on its neighbours' geometry; in another batch, in another lane, it is the same solve
    (to the tolerance of test_batch_independence in tests/test_gpu_obstacles.py)"""
    B, N, K = 6, 30, 3
    prob, q, xi, us, obs = workloads.se3_moving_obstacle_field(B, K, N=N)
    lam, imu = _mults(B, N, K, 2)
    kw = dict(mode="ms", n_iterations=8, line_search=True)
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu)
    r = s.fit_batch(q, xi, us, **kw)
    other = obs.copy()
    keep = [1, 5]
    rng = np.random.default_rng(8)
    for b in set(range(B)) - set(keep):
        other[b, ..., :3] += rng.normal(size=(N + 1, K, 3))
        other[b, ..., 3] *= rng.uniform(0.5, 2.0, (N + 1, K))
    s.set_al_obstacles(other, lam, imu)
    r1 = s.fit_batch(q, xi, us, **kw)
    s.set_al_obstacles(None)
    assert_bitwise(r, r1, keep, keep, "other neighbours")
    assert not torch.equal(bits(r.us[0]), bits(r1.us[0]))
    sub = [5, 1, 5]  # another batch size, another lane
    s3 = BatchedTrackingILQR(prob, 3)
    s3.set_al_obstacles(obs[sub], lam[sub].contiguous(), imu[sub].contiguous())
    r3 = s3.fit_batch(q[sub], xi[sub], us[sub], **kw)
    s3.set_al_obstacles(None)
    for j, b in enumerate(sub):
        x, y = r.us[b].cpu().numpy(), r3.us[j].cpu().numpy()
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
        assert int(r.iters[b]) == int(r3.iters[j])


FLEET = dict(tol_constr=1e-3, n_al_iters=12, n_ilqr_iters=30)


def test_plan_fleet():
    """se3_crossing_fleet(F=2, G=3, N=40, separation=0.3) at the workload's default seed.  On the mirror's host path alone
    (tests/moving.py host_fleet) both fleets stay within the cap of 12 outer iterations: fleet 0 needs 1, 8, 8, fleet 1
    needs 1, 8, 8."""
    F, G, N, sep = 2, 3, 40, 0.3
    prob, q, xi, us, q_ref, xi_ref = workloads.se3_crossing_fleet(F, G, N=N, separation=sep)
    s = BatchedTrackingILQR(prob, F * G)
    res, info = s.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, **FLEET)
    print("min_separation", info["min_separation"].tolist(), "outer_iterations", info["outer_iterations"],
          "max_violation", info["max_violation"].tolist())
    assert info["al_converged"].shape == (F * G,) and bool(info["al_converged"].all())
    assert len(info["outer_iterations"]) == G and max(info["outer_iterations"]) <= 12
    assert info["min_separation"].shape == (F,) and info["max_violation"].shape == (F * G,)
    assert bool((info["min_separation"] >= np.sqrt(sep ** 2 - 1e-3)).all())
    # min_separation is what it says: over knots and pairs of the final plans
    t = res.xs_q[:, :, :3, 3].cpu().numpy().reshape(F, G, N + 1, 3)
    want = [min(np.linalg.norm(t[f, a] - t[f, b], axis=-1).min() for a in range(G) for b in range(a)) for f in range(F)]
    assert np.allclose(info["min_separation"].cpu().numpy(), want, rtol=1e-12, atol=0)
    # member 0 plans as if alone
    plain = s.fit_batch(q[0::G], xi[0::G], us[0::G], mode="ms", n_iterations=30, q_ref=q_ref[0::G], xi_ref=xi_ref[0::G])
    assert_bitwise(res, plain, slice(0, None, G), slice(None), "member 0")
    # the negative control: without the constraint the members pass too close
    free = s.fit_batch(q, xi, us, mode="ms", n_iterations=30, q_ref=q_ref, xi_ref=xi_ref)
    t = free.xs_q[:, :, :3, 3].cpu().numpy().reshape(F, G, N + 1, 3)
    for f in range(F):
        assert min(np.linalg.norm(t[f, a] - t[f, b], axis=-1).min() for a in range(G) for b in range(a)) < 0.2


def test_plan_fleet_argument_errors():
    F, G, N = 2, 3, 20
    prob, q, xi, us, q_ref, xi_ref = workloads.se3_crossing_fleet(F, G, N=N)
    s = BatchedTrackingILQR(prob, F * G)
    with pytest.raises(ValueError, match="fleets"):
        s.plan_fleet(q, xi, us, q_ref, xi_ref, 4, 0.3)            # B % fleet
    with pytest.raises(ValueError, match="exceed"):
        s.plan_fleet(q, xi, us, q_ref, xi_ref, G, 0.3, obstacles=np.ones((15, 4)))  # K0 + fleet - 1 = 17
    assert s._obs is None
