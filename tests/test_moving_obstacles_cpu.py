"""Moving keep-out spheres without a GPU: the C ABI's size query and argument errors, the host checks of the per-knot form, the
two seeded workloads, MovingSphereObstacleConstraint's g_x against central differences, inflate_obstacles, and the method
itself -- prioritised deconfliction of two crossing members -- on the mirror's host generic path."""
import ctypes

import numpy as np
import pytest

from trajectory_optimization_matrix_lie_groups_amd import _capi, inflate_obstacles, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import BatchedTrackingILQR
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_constraints import (MovingSphereObstacleConstraint,
                                                                                            SphereObstacleConstraint)
from tests.moving import g_per_knot, host_fleet

_se3_exp = workloads._se3_exp


def test_size_query_and_argument_errors_without_a_handle():
    lib = _capi.load()
    p = _capi.Problem()
    p.kind, p.m, p.N, p.dt = _capi.DYN_SE3, 6, 40, 0.05
    p.J[0] = p.J[7] = p.J[14] = p.J[21] = p.J[28] = p.J[35] = 1.0
    ref = ctypes.byref(p)
    assert lib.tolg_obstacles_moving_bytes(ref, 5, 3) == 41 * 4 * 3 * 8 * 8  # Bp = 8
    assert lib.tolg_obstacles_moving_bytes(ref, 5, 3) == 41 * lib.tolg_obstacles_bytes(ref, 5, 3)
    p.N = 200
    assert lib.tolg_obstacles_moving_bytes(ref, 4096, 8) == 201 * 4 * 8 * 4096 * 8  # the 211 MB of include/tolg.h
    for K in (0, _capi.MAX_OBSTACLES + 1):
        assert lib.tolg_obstacles_moving_bytes(ref, 4, K) == 0
    assert lib.tolg_obstacles_moving_bytes(ref, 0, 1) == 0
    p.kind = _capi.DYN_SO3
    assert lib.tolg_obstacles_moving_bytes(ref, 4, 1) == 0
    p.kind, p.m = _capi.DYN_DRONE, 4
    assert lib.tolg_obstacles_moving_bytes(ref, 4, 1) == 201 * 4 * 4 * 8
    p.dt = -1.0
    assert lib.tolg_obstacles_moving_bytes(ref, 4, 1) == 0
    assert lib.tolg_set_al_obstacles_moving(None, 1, 1, None, None, None, None, 0, None) == -1
    one = (ctypes.c_double * 8)()
    assert lib.tolg_set_al_obstacles_moving(None, 1, 1, one, one, one, one, 64, None) == -1


class _HostOnly(BatchedTrackingILQR):
    """_check_obstacles needs the problem and N only: no handle, no GPU"""

    def __init__(self, problem):
        self.problem, self.N = problem, problem.N


def test_check_obstacles_on_the_per_knot_form():
    B, N, K = 3, 20, 2
    prob, *_, obs = workloads.se3_moving_obstacle_field(B, K, N=N)
    s = _HostOnly(prob)
    Bc, a = s._check_obstacles(None, obs)
    assert Bc == B and a.shape == (B, N + 1, K, 4) and np.array_equal(a, obs)
    assert s._check_obstacles(B, obs)[0] == B
    with pytest.raises(ValueError, match="shape"):
        s._check_obstacles(B, obs[:, :N])                # N knots
    with pytest.raises(ValueError, match="shape"):
        s._check_obstacles(B + 1, obs)                   # another batch
    with pytest.raises(ValueError, match="shape"):
        s._check_obstacles(B, obs[..., :3])
    bad = obs.copy()
    bad[1, 7, 1, 3] = 0.0
    with pytest.raises(ValueError, match="radius"):
        s._check_obstacles(B, bad)                       # a zero radius at one knot
    bad = obs.copy()
    bad[2, N, 0, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        s._check_obstacles(B, bad)
    with pytest.raises(ValueError, match="K = 17"):
        s._check_obstacles(B, np.ones((B, N + 1, 17, 4)))
    with pytest.raises(ValueError, match="translation"):
        _HostOnly(workloads.so3_tracking(2, N=N)[0])._check_obstacles(2, np.ones((2, N + 1, 1, 4)))
    # the static forms go on as before
    assert s._check_obstacles(B, obs[0, 0])[1].shape == (B, K, 4) and s._check_obstacles(None, obs[:, 0])[1].shape == (B, K, 4)


def test_moving_field_is_seeded_differs_per_trajectory_and_violates_on_the_path():
    a = workloads.se3_moving_obstacle_field(3, 4, N=40, seed=5)
    b = workloads.se3_moving_obstacle_field(3, 4, N=40, seed=5)
    c = workloads.se3_moving_obstacle_field(3, 4, N=40, seed=6)
    obs = a[4]
    assert np.array_equal(obs, b[4]) and not np.array_equal(obs, c[4])
    assert obs.shape == (3, 41, 4, 4) and np.all(obs[..., 3] > 0)
    assert not np.array_equal(obs[0], obs[1])
    v = np.diff(obs[..., :3], axis=1)
    assert np.abs(v - v[:, :1]).max() < 1e-12 and np.all(np.linalg.norm(v[:, 0], axis=-1) > 0)  # a constant velocity, not zero
    assert np.array_equal(obs[..., 3], np.broadcast_to(obs[:, :1, :, 3], obs.shape[:3]))
    g = g_per_knot(np.broadcast_to(a[0].q_ref, (3,) + a[0].q_ref.shape), obs)
    assert np.all(g.max(axis=1) > 0)                    # the reference path violates every sphere
    assert np.all(g[:, 0] < 0) and np.all(g[:, -1] < 0)  # start and end clear
    # each sphere is at its static centre at the knot of the path nearest to it
    static = workloads.se3_obstacle_field(3, 4, N=40, seed=5)[4]
    t = a[0].q_ref[:, :3, 3]
    for bb in range(3):
        for k in range(4):
            i0 = int(np.argmin(np.sum((t - static[bb, k, :3]) ** 2, axis=1)))
            assert np.allclose(obs[bb, i0, k], static[bb, k], rtol=0, atol=1e-14)


def test_crossing_fleet_is_seeded_and_its_members_cross():
    F, G, N, sep = 2, 3, 40, 0.3
    a = workloads.se3_crossing_fleet(F, G, N=N, separation=sep, seed=5)
    b = workloads.se3_crossing_fleet(F, G, N=N, separation=sep, seed=5)
    c = workloads.se3_crossing_fleet(F, G, N=N, separation=sep, seed=6)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[1], c[1])
    prob, q, xi, us, q_ref, xi_ref = a
    assert q.shape == (6, 4, 4) and xi.shape == (6, 6) and us.shape == (6, N, 6) and q_ref.shape == (6, N + 1, 4, 4)
    base = workloads.se3_tracking(F, N=N, R_scale=1e-3, seed=5)
    assert np.array_equal(q[0], base[1][0]) and np.array_equal(q_ref[0], prob.q_ref) and np.array_equal(q_ref[3], prob.q_ref)
    assert not np.array_equal(q[0], q[3]) and not np.array_equal(q[1], q[4])  # the fleets start differently
    t = q_ref[:, :, :3, 3]
    mid = t[0, N // 2]
    for p in range(G):
        # the middle knots lie above each other, 0.3 sep apart; the paths are rotated by p pi / G about z
        assert np.allclose(t[p, N // 2], mid + [0, 0, 0.3 * sep * p], atol=1e-12)
        d0, dp = t[0, N // 2 + 1] - t[0, N // 2], t[p, N // 2 + 1] - t[p, N // 2]
        assert dp[2] == pytest.approx(d0[2], abs=1e-12)
        ang = np.arctan2(dp[1], dp[0]) - np.arctan2(d0[1], d0[0])
        assert np.cos(ang - p * np.pi / G) == pytest.approx(1.0, abs=1e-12)
        assert np.array_equal(xi_ref[p], prob.xi_ref)
        # g_p q_ref is a rigid motion of the reference: the relative poses are the reference's
        rel = np.linalg.inv(q_ref[p, 3]) @ q_ref[p, 4]
        assert np.allclose(rel, np.linalg.inv(prob.q_ref[3]) @ prob.q_ref[4], atol=1e-12)
    assert np.linalg.norm(t[1] - t[0], axis=-1).min() < sep and np.linalg.norm(t[2] - t[1], axis=-1).min() < sep


def _state(seed):
    rng = np.random.default_rng(seed)
    X = _se3_exp(np.r_[rng.normal(size=3) * 0.7, rng.normal(size=3)])
    return [X, rng.normal(size=6)]


def _perturbed(x, j, h):
    """x (+) h e_j in the error coordinates of l_x: pose X Exp(h e_j) for j < 6, twist xi + h e_{j-6} otherwise (the
    differencing of tests/test_obstacles_cpu.py)"""
    X, xi = np.array(x[0]), np.array(x[1])
    if j < 6:
        d = np.zeros(6)
        d[j] = h
        X = X @ _se3_exp(d)
    else:
        xi[j - 6] += h
    return [X, xi]


def _central(f, x, h=1e-6):
    return np.stack([(np.asarray(f(_perturbed(x, j, h))) - np.asarray(f(_perturbed(x, j, -h)))) / (2 * h) for j in range(12)],
                    axis=-1)


def test_moving_g_x_against_central_differences_at_two_knots():
    N, K = 9, 3
    rng = np.random.default_rng(2)
    x = _state(1)
    centers = x[0][:3, 3] + rng.normal(size=(N + 1, K, 3)) * 0.4
    radii = rng.uniform(0.2, 0.6, (N + 1, K))
    c = MovingSphereObstacleConstraint(centers, radii)
    u = np.zeros(6)
    assert c.constr_size == K and c.obstacles().shape == (N + 1, K, 4)
    assert np.array_equal(c.obstacles()[..., :3], centers) and np.array_equal(c.obstacles()[..., 3], radii)
    for i in (2, N):
        gx = c.g_x(x, u, i)
        assert gx.shape == (K, 12) and np.all(gx[:, :3] == 0) and np.all(gx[:, 6:] == 0)
        assert np.abs(_central(lambda y: c.g(y, u, i), x) - gx).max() < 1e-7 * max(1.0, np.abs(gx).max())
        s = SphereObstacleConstraint(centers[i], radii[i])  # knot i's geometry, and no other knot's
        assert np.array_equal(c.g(x, u, i), s.g(x, u, i)) and np.array_equal(gx, s.g_x(x, u, i))
    assert not np.array_equal(c.g(x, u, 2), c.g(x, u, N))
    assert np.allclose(c.g(x, None, N, terminal=True), c.g(x, u, N))  # terminal included
    assert c.g_u(x, u, 2).shape == (K, 6) and not c.g_u(x, u, 2).any()
    shared = MovingSphereObstacleConstraint(centers, radii[0])  # radii [K]: the same at every knot
    assert np.array_equal(shared.obstacles()[..., 3], np.broadcast_to(radii[0], (N + 1, K)))
    with pytest.raises(ValueError):
        MovingSphereObstacleConstraint(centers[0], radii[0])
    with pytest.raises(ValueError):
        MovingSphereObstacleConstraint(centers, radii[:, :2])


def test_inflate_obstacles():
    B, N, K = 2, 5, 3
    rng = np.random.default_rng(3)
    xs_q = np.broadcast_to(np.eye(4), (B, N + 1, 4, 4)).copy()
    xs_q[..., :3, 3] = rng.normal(size=(B, N + 1, 3))
    static = np.concatenate([rng.normal(size=(B, K, 3)), rng.uniform(0.2, 0.5, (B, K, 1))], axis=-1)
    moving = np.concatenate([rng.normal(size=(B, N + 1, K, 3)), rng.uniform(0.2, 0.5, (B, N + 1, K, 1))], axis=-1)
    sigma, kappa = 0.07, 2.5
    iso = np.broadcast_to(sigma ** 2 * np.eye(3), (B, N + 1, 3, 3))
    for field in (static[0], static, moving):
        out = inflate_obstacles(field, xs_q, iso, kappa)
        full = np.broadcast_to(field if field.ndim == 4 else field[None, None] if field.ndim == 2 else field[:, None],
                               (B, N + 1, K, 4))
        assert out.shape == (B, N + 1, K, 4) and np.array_equal(out[..., :3], full[..., :3])
        assert np.allclose(out[..., 3], full[..., 3] + kappa * sigma, rtol=1e-14, atol=0)  # isotropic: r + kappa sigma everywhere
    # rank one: sigma^2 a a^T gives the projection of a on the line from the centre to the nominal position
    a = rng.normal(size=(B, N + 1, 3))
    a /= np.linalg.norm(a, axis=-1, keepdims=True)
    out = inflate_obstacles(moving, xs_q, sigma ** 2 * a[..., :, None] * a[..., None, :], kappa)
    n = xs_q[..., :3, 3][:, :, None, :] - moving[..., :3]
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    proj = np.abs(np.einsum("bikc,bic->bik", n, a))
    assert np.allclose(out[..., 3], moving[..., 3] + kappa * sigma * proj, rtol=1e-12, atol=1e-15)
    assert proj.min() < 0.2 and proj.max() > 0.9  # directions along the line and across it
    import torch
    assert np.array_equal(inflate_obstacles(torch.as_tensor(moving), torch.as_tensor(xs_q), torch.as_tensor(iso.copy()), kappa),
                          inflate_obstacles(moving, xs_q, iso, kappa))
    with pytest.raises(ValueError):
        inflate_obstacles(moving[:, :N], xs_q, iso, kappa)


def test_prioritised_deconfliction_on_the_host_path():
    """Two members crossing at 90 degrees (se3_crossing_fleet(1, 2), N = 40, separation 0.3): member 1 keeps out of one moving
    sphere on member 0's solved positions.  30 MS iterations per outer iteration, the outer rule of al_fit_batch, tol 1e-3.
    Measured when the method was proposed: unconstrained separation 0.15 at most, 7 outer iterations."""
    prob, q, xi, _, q_ref, xi_ref = workloads.se3_crossing_fleet(1, 2, N=40, separation=0.3)
    free, sep, outers = host_fleet(prob, q, xi, q_ref, xi_ref, 0.3, n_al=12, n_ilqr=30, tol=1e-3)
    print("unconstrained separation %.4f, planned %.4f, outer iterations %s" % (free, sep, outers))
    assert free < 0.2                                    # without the constraint the members pass too close
    assert outers[0] == 1 and outers[1] is not None and outers[1] <= 12
    assert sep ** 2 > 0.3 ** 2 - 1e-3                    # max g < tol at every knot
