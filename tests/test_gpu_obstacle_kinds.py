"""Constraint kinds beyond the keep-out sphere (tolg_set_al_obstacle_kinds): keep-in spheres, half-spaces and vertical columns in
the slots of tolg_set_al_obstacles*, against the NumPy restatement of tests/kinds.py.

1. kind 0 in every slot, given explicitly or as NULL, is bitwise the handle on which the call was never made;
2. the linearisation's J, l_x[3:6] and l_xx[3:6, 3:6] move by the restated terms of every kind, nothing else moves at all;
3. zero multipliers give the bits of the solve without constraints;
4. fixed multipliers: the GPU solve against the mirror's host generic path on PositionObstacleConstraint;
5. tolg_al_update_state and tolg_al_mpc_step on the rows of every kind;
6. the clearance of the limited policy rollout per kind, across the second trip of its four-slot loop;
7. al_fit_batch and mpc on the corridor workload;
8. the contract of the call.

Tolerances.  The linearisation terms, the multipliers and the largest violation carry test_gpu_obstacles' bounds (relative
1e-12 of the largest expected entry, floor 1; multipliers rtol 1e-12 with the 1e-15 absolute floor of
test_outer_update_against_a_restatement: lambda + I g cancels).  The clearance |d| - r is a difference of two lengths of the
size of the scene (here <= 10), each good to a few ulp: 1e-12 of max(1, |clearance|)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_constraints import PositionObstacleConstraint
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_controller import (iLQR_Tracking_SE3,
                                                                                           iLQR_Tracking_SE3_MS)
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_cost import ALConstrainedCost
from tests import kinds as kd
from tests.mpc_al import al_mpc_step_restated, g_box, shifted
from tests.restate import MyCost, MyDynamics
from tests.support import ZERO, dense_fixed_block, host, pert, same

pytestmark = pytest.mark.gpu
f64 = dict(dtype=torch.float64, device="cuda:0")
P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
MIXED = (kd.HALF_SPACE, kd.SPHERE, kd.KEEP_IN, kd.COLUMN, kd.COLUMN, kd.HALF_SPACE)   # K = 6, two kinds twice
RT, AT = 1e-12, 1e-15

# test_gpu_obstacles.MODES
MODES = [dict(mode="ms", n_iterations=10, tol_grad_norm=0.0, tol_d_norm=0.0),
         dict(mode="ms", n_iterations=10, tol_grad_norm=0.0, tol_d_norm=0.0, schedule="split"),
         dict(mode="ms", n_iterations=15, line_search=True),
         dict(mode="ss", n_iterations=15),
         dict(mode="ms", n_iterations=15, line_search=True, rollout="linear")]


def _mults(B, N, K, seed, lam=1.0, imu=20.0):
    rng = np.random.default_rng(seed)
    return (torch.as_tensor(rng.uniform(0.0, lam, (B, N + 1, K)), **f64).contiguous(),
            torch.as_tensor(rng.uniform(0.0, imu, (B, N + 1, K)), **f64).contiguous())


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rel * max(1.0, np.abs(b).max())


def _raw_kinds(s, kinds, K=None):
    """tolg_set_al_obstacle_kinds itself, past the binding's bookkeeping; kinds None: NULL"""
    K = len(kinds) if K is None else K
    arr = None if kinds is None else (C.c_int32 * len(kinds))(*kinds)
    with torch.cuda.device(s.device):
        return s.lib.tolg_set_al_obstacle_kinds(s._h, K, arr, s._stream())


def _model(name, B, N):
    if name == "drone":
        prob, q, xi, us = workloads.drone_tracking(B, N=N)
    else:
        prob, q, xi, us = workloads.se3_tracking(B, N=N)
        if name == "rigidbody":
            prob = TrackingProblem("rigidbody", prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
        elif name == "dense":
            prob = dense_fixed_block(prob)
    return prob, q, xi, us


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(mode="ms", n_iterations=10, **ZERO), dict(mode="ms", n_iterations=10, line_search=True),
                                dict(mode="ss", n_iterations=10)])
def test_kind_zero_is_the_path_without_the_call(kw):
    B, N, K = 6, 40, 3
    prob, q, xi, us, obs = workloads.se3_obstacle_field(B, K, N=N)
    lam, imu = _mults(B, N, K, 5)
    out = []
    for call in ("none", "zeros", "null"):
        s = BatchedTrackingILQR(prob, B)
        s.set_al_obstacles(obs, lam, imu)
        if call != "none":
            assert _raw_kinds(s, None if call == "null" else (0,) * K, K) == 0
        out.append(s.fit_batch(q, xi, us, **kw))
        s.set_al_obstacles(None)
    for r in out[1:]:
        for f in ("us", "xs_q", "J_hist", "iters"):
            assert same(getattr(out[0], f), getattr(r, f)), f
    # ... and the spheres did something: the call is not compared on a solve that ignores them
    s = BatchedTrackingILQR(prob, B)
    assert not same(s.fit_batch(q, xi, us, **kw).us, out[0].us)


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("name", ["se3", "rigidbody", "drone", "dense"])
def test_linearisation_terms_per_kind(name, moving, pt):
    B, N = 5, 30
    prob, *_ = _model(name, B, N)
    rng = np.random.default_rng(3)
    span = np.ptp(prob.q_ref[:, :3, 3], axis=0).max()
    xs_q = np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy()
    xs_q[..., :3, 3] += 0.05 * span * rng.normal(size=(B, N + 1, 3))
    xs_xi = np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape) + 0.1 * rng.normal(size=(B, N + 1, 6))
    us = 0.1 * rng.normal(size=(B, N, prob.m))
    obs = kd.mixed_slots(xs_q[..., :3, 3], MIXED, seed=7, moving=moving)
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
    lam, imu = _mults(B, N, len(MIXED), 5)
    s.set_al_obstacles(obs, lam, imu, kinds=MIXED)
    b = s.linearize_backward(xs_q, xs_xi, us, **kw)
    s.set_al_obstacles(None)
    g, l, lx, lxx = kd.terms(xs_q, obs, MIXED, host(lam), host(imu))
    for q in range(4):   # every kind on both sides of its surface
        gq = g[..., [k for k, x in enumerate(MIXED) if x == q]]
        assert (gq > 0).any() and (gq < 0).any(), q
    assert _close(host(b["J"]) - host(a["J"]), l.sum(axis=1))
    assert _close(host(b["lx"])[..., 3:6] - host(a["lx"])[..., 3:6], lx)
    assert torch.equal(b["lx"][..., :3], a["lx"][..., :3]) and torch.equal(b["lx"][..., 6:], a["lx"][..., 6:])
    assert _close(host(b["lxx11"])[..., 3:, 3:] - host(a["lxx11"])[..., 3:, 3:], lxx)
    assert torch.equal(b["lxx11"][..., :3, :], a["lxx11"][..., :3, :]) and torch.equal(b["lxx11"][..., 3:, :3], a["lxx11"][..., 3:, :3])
    # the kinds are read: the same fields as keep-out spheres give other terms
    assert not _close(l.sum(axis=1), kd.terms(xs_q, obs, (0,) * 6, host(lam), host(imu))[1].sum(axis=1), rel=1e-3)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", MODES)
def test_zero_multipliers_change_nothing(kw):
    B, N = 6, 60
    prob, q, xi, us, obs, kinds = workloads.se3_corridor(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.fit_batch(q, xi, us, **kw)
    z = torch.zeros(B, N + 1, obs.shape[1], **f64)
    s.set_al_obstacles(obs, z, z.clone(), kinds=kinds)
    r1 = s.fit_batch(q, xi, us, **kw)
    s.set_al_obstacles(None)
    for f in ("xs_q", "xs_xi", "us", "J_hist", "iters", "status"):
        a, b = getattr(r0, f), getattr(r1, f)
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)), f


# 4 -------------------------------------------------------------------------------------------------------------------
def _host_solve(prob, x0_q, x0_xi, us0, obs, kinds, lam, imu, kw):
    """tests.checks.host_solve with PositionObstacleConstraint in place of the sphere constraint: (J per iteration, us)"""
    op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
    al = ALConstrainedCost(MyCost(op, prob.m), PositionObstacleConstraint(obs, kinds), prob.N)
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
            ctl = iLQR_Tracking_SE3_MS(MyDynamics(op, prob.m), al, prob.N, prob.q_ref, prob.xi_ref, rollout=rollout,
                                       line_search=kw.get("line_search", False))
        else:
            ctl = iLQR_Tracking_SE3(MyDynamics(op, prob.m), al, prob.N, rollout=rollout)
        xs, us, *_ = ctl.fit([x0_q, x0_xi], us0, n_iterations=kw["n_iterations"], tol_grad_norm=0.0, on_iteration=cb)
    return np.array(J), us


@pytest.mark.parametrize("kw", [dict(mode="ms", n_iterations=6), dict(mode="ms", n_iterations=6, line_search=True),
                                dict(mode="ss", n_iterations=6), dict(mode="ms", n_iterations=6, rollout="linear")])
def test_fixed_multiplier_parity_with_the_host_generic_path(kw):
    B, N = 3, 40
    obs = workloads.se3_corridor(B, N=N, seed=11)[4]
    prob, q, xi, us0 = workloads.se3_tracking(B, N=N, R_scale=1e-3, seed=11)
    lam, imu = _mults(B, N, 6, 9, lam=0.5, imu=5.0)
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu, kinds=kd.CORRIDOR)
    r = s.fit_batch(q, xi, us0, tol_grad_norm=0.0, tol_d_norm=0.0, check_every=0, **kw)
    s.set_al_obstacles(None)
    for b in range(B):
        J, us = _host_solve(prob, q[b], xi[b], us0[b], obs[b], kd.CORRIDOR, host(lam[b]), host(imu[b]), kw)
        n = int(r.iters[b])
        # (a merit search that finds no step ends the solve on both sides: the same count, ST_NODESCENT here)
        assert n == len(J) and int(r.status[b]) == (_capi.ST_OK if n == kw["n_iterations"] else _capi.ST_NODESCENT)
        assert np.abs(host(r.J_hist[b, :n]) / J - 1).max() < 1e-9
        assert np.abs(host(r.us[b]) - us).max() < 1e-6 * max(1.0, np.abs(us).max())


# 5 -------------------------------------------------------------------------------------------------------------------
def _corridor_step_inputs(B, N, seed):
    """The corridor mix on positions scattered about the reference path, so that the rows have both signs"""
    prob, q, xi, us0, obs, _ = workloads.se3_corridor(B, N=N)
    rng = np.random.default_rng(seed)
    xs_q = np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy()
    xs_q[..., :3, 3] += 0.2 * rng.normal(size=(B, N + 1, 3))
    us = rng.normal(size=(B, N, prob.m)) * 2.0
    return prob, xs_q, us, obs


def _random_mults(rng, B, rows, W):
    """Multipliers with some lambda = 0 and some I_mu = 0"""
    return [torch.as_tensor(rng.uniform(0.0, hi, (B, rows, W)) * (rng.uniform(size=(B, rows, W)) > 0.3), **f64).contiguous()
            for hi in (1.0, 20.0)]


@pytest.mark.parametrize("box", [False, True])
def test_outer_update_per_kind(box):
    B, N, mu0, tol = 2, 20, 0.5, 1e-2
    prob, xs_q, us, obs = _corridor_step_inputs(B, N, 1)
    rng = np.random.default_rng(2)
    lam, imu = _random_mults(rng, B, N + 1, 6)
    lam0, imu0 = host(lam).copy(), host(imu).copy()
    g = kd.g_rows(xs_q, obs, kd.CORRIDOR)
    for q in range(4):
        gq = g[..., [k for k, x in enumerate(kd.CORRIDOR) if x == q]]
        assert (gq > tol).any() and (gq < 0).any(), q
    s = BatchedTrackingILQR(prob, B)
    s.set_al_obstacles(obs, lam, imu, kinds=kd.CORRIDOR)
    mv = g.max(axis=(1, 2))
    if box:
        lb, ub = -np.ones(prob.m), np.ones(prob.m)
        bl, bi = _random_mults(rng, B, N, 2 * prob.m)
        bl0, bi0 = host(bl).copy(), host(bi).copy()
        s.set_al(lb, ub, bl, bi)
        gb = g_box(us, lb, ub)
        mv = np.maximum(mv, np.maximum(gb.max(axis=(1, 2)), 0.0))
    mu = torch.full((B,), mu0, **f64)
    maxviol, alconv = torch.zeros(B, **f64), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    xq_d, us_d = torch.as_tensor(xs_q, **f64).reshape(B, N + 1, 16).contiguous(), torch.as_tensor(us, **f64).contiguous()
    s._call("tolg_al_update_state", B, P(xq_d), P(us_d), P(mu), 10.0, 1e8, tol, P(maxviol), P(alconv))
    s.set_al_obstacles(None)
    s.set_al(None)
    ln, im = kd.update(g, lam0, imu0, mu0)
    assert np.allclose(host(maxviol), mv, rtol=RT, atol=0)
    assert np.allclose(host(lam), ln, rtol=RT, atol=AT) and np.array_equal(host(imu), im)
    if box:
        lb_, ib_ = kd.update(gb, bl0, bi0, mu0)
        assert np.allclose(host(bl), lb_, rtol=RT, atol=AT) and np.array_equal(host(bi), ib_)
    assert np.array_equal(host(mu), np.full(B, 10 * mu0)) and not host(alconv).any()
    # the rows are those of the kinds: as keep-out spheres the same fields give another update
    assert not np.allclose(kd.update(kd.g_rows(xs_q, obs, (0,) * 6), lam0, imu0, mu0)[0], ln)


@pytest.mark.parametrize("box", [False, True])
def test_mpc_step_per_kind(box):
    B, N, mu0, tol = 2, 20, 0.5, 1e-2
    prob, xs_q, us, obs = _corridor_step_inputs(B, N, 3)
    rng = np.random.default_rng(4)
    lam0, imu0 = _random_mults(rng, B, N + 1, 6)
    g = kd.g_rows(xs_q, obs, kd.CORRIDOR)
    rows_o = (g, host(lam0), host(imu0))
    rows_b = None
    if box:
        lb, ub = -np.ones(prob.m), np.ones(prob.m)
        bl0, bi0 = _random_mults(rng, B, N, 2 * prob.m)
        rows_b = (g_box(us, lb, ub), host(bl0), host(bi0))
    s = BatchedTrackingILQR(prob, B)
    xq_d, us_d = torch.as_tensor(xs_q, **f64), torch.as_tensor(us, **f64)
    got = {}
    for shift in (0, 1):
        lam, imu = lam0.clone(), imu0.clone()
        s.set_al_obstacles(obs, lam, imu, kinds=kd.CORRIDOR)
        if box:
            bl, bi = bl0.clone(), bi0.clone()
            s.set_al(lb, ub, bl, bi)
        mu = torch.full((B,), mu0, **f64)
        mv = s.al_mpc_step(xq_d, us_d if box else None, mu, 10.0, 1e8, tol, shift)
        s.set_al(None)
        s.set_al_obstacles(None)
        e_mv, e_mu, e_box, e_obs = al_mpc_step_restated(np.full(B, mu0), 10.0, 1e8, tol, shift, rows_b, rows_o)
        assert np.allclose(host(mv), e_mv, rtol=RT, atol=0) and np.array_equal(host(mu), e_mu)
        assert np.allclose(host(lam), e_obs[0], rtol=RT, atol=AT) and np.array_equal(host(imu), e_obs[1])
        if box:
            assert np.allclose(host(bl), e_box[0], rtol=RT, atol=AT) and np.array_equal(host(bi), e_box[1])
        got[shift] = (host(lam), host(imu)) + ((host(bl), host(bi)) if box else ())
    for a0, a1 in zip(got[0], got[1]):   # the shift is data movement: the unshifted update, shifted on the host
        assert np.array_equal(shifted(a0), a1)


# 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moving", [False, True])
def test_clearance_per_kind(moving):
    B, S, N = 3, 4, 30
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    nom = s.fit_batch(q, xi, us, mode="ms", n_iterations=8, **ZERO)
    slots = kd.mixed_slots(host(nom.xs_q)[..., :3, 3], MIXED, seed=13, moving=moving)
    dx0, w = pert(B, S, N, seed=11)
    s.set_al_obstacles(slots, kinds=MIXED)
    try:
        p = s.policy_rollout(dx0, w, trajectories=True, clearance=True)
    finally:
        s.set_al_obstacles(None)
    t = host(p.xs_q)[..., :3, 3]
    c, k = host(p.clearance), host(p.clearance_knot)
    assert (host(p.status) == _capi.ST_OK).all()
    clear_cut, last_trip = 0, 0
    for b in range(B):
        for j in range(S):
            want, knot, runner_up = kd.clearance_of(t[b, j], slots[b], MIXED)
            assert abs(c[b, j] - want) <= 1e-12 * max(1.0, abs(want)), (b, j, c[b, j], want)
            if runner_up - want > 1e-9:
                clear_cut += 1
                assert k[b, j] == knot, (b, j)
            per_slot = kd.rows(t[b, j], slots[b][None] if slots[b].ndim == 2 else slots[b], MIXED)[2].min(axis=0)
            last_trip += int(np.argmin(per_slot) >= 4)
    assert 4 * clear_cut >= 3 * B * S
    assert (c < 0).any()
    assert last_trip > 0   # some minimum lies in the partial second trip of the four-slot loop
    # as keep-out spheres the same slots give another clearance (a half-space's offset is no radius: made one)
    sph = slots.copy()
    sph[..., 3] = np.abs(sph[..., 3]) + 0.1
    s.set_al_obstacles(sph)
    try:
        p0 = s.policy_rollout(dx0, w, clearance=True)
    finally:
        s.set_al_obstacles(None)
    assert not same(p0.clearance, p.clearance)


# 7 -------------------------------------------------------------------------------------------------------------------
def test_corridor_end_to_end():
    B, N, tol = 4, 40, 1e-2
    prob, q, xi, us, obs, kinds = workloads.se3_corridor(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.fit_batch(q, xi, us, n_iterations=100, line_search=True)
    g0 = kd.g_rows(host(r0.xs_q), obs, kd.CORRIDOR)
    for x in range(4):   # the unconstrained solve breaks every kind
        assert (g0[..., [k for k, y in enumerate(kd.CORRIDOR) if y == x]].max(axis=(1, 2)) > tol).any(), x
    res, info = s.al_fit_batch(q, xi, us, n_al_iters=20, n_ilqr_iters=100, obstacles=obs, obstacle_kinds=kinds, tol_constr=tol,
                               line_search=True)
    conv = host(info["al_converged"]).astype(bool)
    g = kd.g_rows(host(res.xs_q), obs, kd.CORRIDOR)
    print("corridor: converged %s, max row %s -> %s" % (conv, g0.max(axis=(1, 2)), g.max(axis=(1, 2))))
    assert conv.any()
    assert np.all(g[conv] < tol)
    assert np.allclose(host(info["max_violation"])[conv], g.max(axis=(1, 2))[conv], rtol=RT, atol=0)
    assert s._obs is None and s._obs_kinds == ()


def test_mpc_reports_the_clearance_of_every_kind():
    B, N, steps = 4, 40, 6
    prob, q, xi, pq, px, t0, noise = workloads.se3_mpc(B, steps, N=N, seed=21)
    idx = np.minimum(np.asarray(t0)[:, None] + np.arange(N + steps + 1)[None], pq.shape[1] - 1)
    t_path = pq[np.arange(B)[:, None], idx][..., :3, 3]   # what the windows of the loop will track
    obs = kd.mixed_slots(t_path, kd.CORRIDOR, seed=17)
    s = BatchedTrackingILQR(prob, B)
    r = s.mpc(q, xi, pq, px, steps, t0=t0, first_iters=20, iters_per_step=5, noise=noise, obstacles=obs,
              obstacle_kinds=workloads.CORRIDOR_KINDS)
    for f in (r.xs_q, r.xs_xi, r.us, r.J, r.max_violation, r.clearance):
        assert torch.isfinite(f).all()
    want = kd.rows(host(r.xs_q)[..., :3, 3], obs[:, None], kd.CORRIDOR)[2].min(axis=-1)
    assert r.clearance.shape == (B, steps + 1) and _close(host(r.clearance), want)
    assert not _close(want, kd.rows(host(r.xs_q)[..., :3, 3], obs[:, None], (0,) * 6)[2].min(axis=-1), rel=1e-3)
    assert s._obs is None and s._obs_kinds == ()


# 8 -------------------------------------------------------------------------------------------------------------------
def test_contract():
    B, N, K = 3, 20, 3
    kinds = (kd.KEEP_IN, kd.HALF_SPACE, kd.COLUMN)
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    rng = np.random.default_rng(0)
    xs_q = np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy()
    xs_q[..., :3, 3] += 0.2 * rng.normal(size=(B, N + 1, 3))
    obs = kd.mixed_slots(xs_q[..., :3, 3], kinds, seed=1)
    s = BatchedTrackingILQR(prob, 4)
    lib, h, st = s.lib, s._h, s._stream()
    xq_d = torch.as_tensor(xs_q, **f64).reshape(B, N + 1, 16).contiguous()
    d = torch.as_tensor(obs, **f64).contiguous()
    d_mov = d[:, None].expand(B, N + 1, K, 4).contiguous()
    d_path = d[:, None].expand(B, N + 3, K, 4).contiguous()
    lam, imu = (torch.zeros(B, N + 1, K, **f64) for _ in range(2))
    buf = torch.empty(lib.tolg_obstacles_moving_bytes(C.byref(s._p), 4, 16) // 8, **f64)
    nb = C.c_size_t(buf.numel() * 8)
    forms = {"static": lambda k, src=d: lib.tolg_set_al_obstacles(h, B, k, P(src), P(lam), P(imu), P(buf), nb, st),
             "moving": lambda k, src=d_mov: lib.tolg_set_al_obstacles_moving(h, B, k, P(src), P(lam), P(imu), P(buf), nb, st),
             "windows": lambda k, src=d_path: lib.tolg_set_al_obstacle_windows(h, B, k, P(src), N + 2, None, 1, P(lam), P(imu),
                                                                               P(buf), nb, st)}
    detach = lambda: lib.tolg_set_al_obstacles(h, 0, 0, None, None, None, None, C.c_size_t(0), None)  # noqa: E731

    def seen():
        """The largest row of what is attached (shift 0, zero multipliers: nothing else moves): which kinds the handle holds"""
        mu, mv = torch.ones(B, **f64), torch.zeros(B, **f64)
        lam.zero_(); imu.zero_()
        assert lib.tolg_al_mpc_step(h, B, P(xq_d), None, P(mu), 10.0, 1e8, 1e-2, P(mv), 0, st) == 0
        return host(mv)

    as_kinds = kd.g_rows(xs_q, obs, kinds).max(axis=(1, 2))
    as_spheres = kd.g_rows(xs_q, obs, (0,) * K).max(axis=(1, 2))
    assert not np.allclose(as_kinds, as_spheres, rtol=1e-3)
    # TOLG_E_ARG
    assert _raw_kinds(s, kinds) == -1                       # nothing attached
    assert forms["static"](K) == 0
    assert np.allclose(seen(), as_spheres, rtol=RT, atol=0)  # never called: keep-out spheres
    assert _raw_kinds(s, kinds[:2]) == -1 and _raw_kinds(s, kinds + (0,)) == -1   # K other than the attached K
    assert _raw_kinds(s, None, K + 1) == -1
    assert _raw_kinds(s, (0, 4, 1)) == -1 and _raw_kinds(s, (0, -1, 1)) == -1    # a kind outside 0..3
    assert np.allclose(seen(), as_spheres, rtol=RT, atol=0)  # a refused call changes nothing
    s.solve_begin(q, xi, us, n_iterations=2)
    assert _raw_kinds(s, kinds) == -1                       # a solve in flight
    s.solve_iterate(2)
    s.solve_end()
    # the held policy is left alone
    K0 = s.gains()["K"].clone()
    assert _raw_kinds(s, kinds) == 0
    assert torch.equal(s.gains()["K"], K0)
    assert np.allclose(seen(), as_kinds, rtol=RT, atol=0)
    # kept over a re-attach with the same K, in each form
    for name, attach in forms.items():
        assert attach(K) == 0, name
        assert np.allclose(seen(), as_kinds, rtol=RT, atol=0), name
    # NULL: keep-out spheres again
    assert _raw_kinds(s, None, K) == 0
    assert np.allclose(seen(), as_spheres, rtol=RT, atol=0)
    # reset by another K, in each form, and by a detach
    two = kd.g_rows(xs_q, obs[:, :2], (0, 0)).max(axis=(1, 2))
    for name in forms:
        assert forms["static"](K) == 0 and _raw_kinds(s, kinds) == 0
        src = {"static": d[:, :2], "moving": d_mov[:, :, :2], "windows": d_path[:, :, :2]}[name].contiguous()
        assert forms[name](2, src) == 0, name
        mu, mv = torch.ones(B, **f64), torch.zeros(B, **f64)
        lam.zero_(); imu.zero_()
        assert lib.tolg_al_mpc_step(h, B, P(xq_d), None, P(mu), 10.0, 1e8, 1e-2, P(mv), 0, st) == 0
        assert np.allclose(host(mv), two, rtol=RT, atol=0), name
        assert forms["static"](K) == 0
        assert np.allclose(seen(), as_spheres, rtol=RT, atol=0), name
    assert _raw_kinds(s, kinds) == 0 and detach() == 0
    assert _raw_kinds(s, kinds) == -1
    assert forms["static"](K) == 0
    assert np.allclose(seen(), as_spheres, rtol=RT, atol=0)
    assert detach() == 0
    torch.cuda.synchronize()


def test_value_errors_before_the_device():
    B, N = 2, 20
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    n = np.array([0.6, 0.0, 0.8])
    good = np.broadcast_to(np.array([[0, 0, 0, 1.0], [0, 0, 0, 9.0], [*n, -2.0], [1, 1, 0, 0.5]]), (B, 4, 4)).copy()
    s.set_al_obstacles(good, kinds=kd.NAMES)
    assert s._obs_kinds == (0, 1, 2, 3)
    s.set_al_obstacles(None)

    def bad(k, col, v):
        a = good.copy()
        a[:, k, col] = v
        return a

    cases = [(good, kd.NAMES[:3]), (good, ("sphere", "keep_in", "half_space", "cone")), (good, (0, 1, 2, 4)),
             (bad(0, 3, 0.0), kd.NAMES), (bad(1, 3, -1.0), kd.NAMES), (bad(3, 3, 0.0), kd.NAMES),
             (bad(2, 0, 0.6 + 1e-8), kd.NAMES), (bad(2, slice(0, 3), 0.0), kd.NAMES)]
    for a, k in cases:
        with pytest.raises(ValueError):
            s.set_al_obstacles(a, kinds=k)
        with pytest.raises(ValueError):
            s.al_fit_batch(q, xi, us, obstacles=a, obstacle_kinds=k)
        path = np.broadcast_to(a[:, None], (B, N + 5, 4, 4)).copy()
        with pytest.raises(ValueError):
            s.set_al_obstacle_windows(path, 0, kinds=k)
        with pytest.raises(ValueError):
            s.set_al_obstacle_windows(torch.as_tensor(path, **f64), 0, kinds=k)
    assert s._obs is None
    with pytest.raises(ValueError):
        s.al_fit_batch(q, xi, us, lb=-np.ones(6), ub=np.ones(6), obstacle_kinds=(0,))
    # a negative offset is a half-space like any other
    s.set_al_obstacle_windows(np.broadcast_to(good[:, None], (B, N + 5, 4, 4)).copy(), 0, kinds=kd.NAMES)
    s.set_al_obstacles(None)
