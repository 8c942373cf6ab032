"""Pose schedules (tolg_set_pose_schedule, pose_scale=) without a GPU: the size query of the packed buffer, the argument errors
that need no handle, the host-side check of a schedule, the gates workload, the window rule, the per-knot restatement the GPU
tests compare against, and the gate property on the mirror's host generic path."""
import ctypes

import numpy as np
import pytest

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import mpc_window_index
from tests.schedule import (distinct_schedule, gather_windows, host_scheduled_solve, knot_ops, lin_scheduled, pose_scaled,
                            restate_value_scheduled)
from tests.restate import restate_value
from tests.support import near, op_of


def test_pose_schedule_bytes_query():
    lib = _capi.load()
    p = _capi.Problem()
    p.kind, p.m, p.N, p.dt = _capi.DYN_SE3, 6, 200, 0.05
    for B in (1, 4, 13, 4096):
        Bp = (B + 3) // 4 * 4
        assert lib.tolg_pose_schedule_bytes(ctypes.byref(p), B) == (200 + 1) * 6 * Bp * 8
    assert lib.tolg_pose_schedule_bytes(ctypes.byref(p), 0) == 0
    assert lib.tolg_pose_schedule_bytes(ctypes.byref(p), -3) == 0
    assert lib.tolg_pose_schedule_bytes(None, 4) == 0
    p.kind, p.m, p.N = _capi.DYN_DRONE, 4, 7
    assert lib.tolg_pose_schedule_bytes(ctypes.byref(p), 13) == 8 * 6 * 16 * 8
    p.kind, p.m = _capi.DYN_SE3, 4  # SE3 dynamics has 6 inputs: an invalid problem
    assert lib.tolg_pose_schedule_bytes(ctypes.byref(p), 16) == 0
    p.kind, p.m, p.dt = _capi.DYN_DRONE, 4, -1.0
    assert lib.tolg_pose_schedule_bytes(ctypes.byref(p), 16) == 0


def test_setters_without_handle_are_argument_errors():
    lib = _capi.load()
    assert lib.tolg_set_pose_schedule(None, 4, None, None, 0, None) == -1
    assert lib.tolg_set_pose_schedule_windows(None, 4, None, 8, None, 0, None, 0, None) == -1


def _fake_solver(N=5, m=6, Q=None, P=None, R=None):
    """the host-side checks alone: no handle, no device"""
    s = object.__new__(BatchedTrackingILQR)
    s.N, s.m = N, m
    ref = np.tile(np.eye(4), (N + 1, 1, 1))
    s.problem = TrackingProblem("se3", np.eye(6), 0.05, np.eye(12) * 2 if Q is None else Q, np.eye(m) * 0.5 if R is None else R,
                                np.eye(12) * 3 if P is None else P, ref, np.zeros((N + 1, 6)))
    return s


def test_check_pose_scale_accepts_the_four_shapes():
    B, N = 4, 5
    s = _fake_solver(N)
    assert s._check_pose_scale(B, None) is None
    full = distinct_schedule(B, N)
    np.testing.assert_array_equal(s._check_pose_scale(B, full), full)
    a = s._check_pose_scale(B, full[1])                 # [N+1, 6]: every trajectory the same
    assert a.shape == (B, N + 1, 6)
    for b in range(B):
        np.testing.assert_array_equal(a[b], full[1])
    a = s._check_pose_scale(B, full[:, :, 2])           # [B, N+1]: one factor for the six coordinates
    assert a.shape == (B, N + 1, 6)
    for k in range(6):
        np.testing.assert_array_equal(a[:, :, k], full[:, :, 2])
    a = s._check_pose_scale(B, full[3, :, 0])           # [N+1]
    assert a.shape == (B, N + 1, 6)
    np.testing.assert_array_equal(a, np.broadcast_to(full[3, :, 0][None, :, None], (B, N + 1, 6)))
    z = np.zeros((B, N + 1, 6))                         # zero switches pose tracking off: legal
    np.testing.assert_array_equal(s._check_pose_scale(B, z), z)
    assert s._check_pose_scale(B, [1.0] * (N + 1)).shape == (B, N + 1, 6)  # a plain sequence
    # B = N + 1 = 6: a (6, 6) array is [N+1, 6]
    s6 = _fake_solver(5)
    sq = distinct_schedule(1, 5)[0]
    np.testing.assert_array_equal(s6._check_pose_scale(6, sq)[4], sq)


def test_check_pose_scale_errors():
    B, N = 4, 5
    s = _fake_solver(N)
    ok = np.ones((B, N + 1, 6))
    for bad in (ok[:, :N], ok[:3], ok[:, :, :5], np.ones((N, 6)), np.ones((B + 1, N + 1)), np.ones(N), np.ones((B, N + 1, 6, 1)),
                np.float64(1.0)):
        with pytest.raises(ValueError):
            s._check_pose_scale(B, bad)
    for v in (np.nan, np.inf, -np.inf, -1e-3):
        a = ok.copy()
        a[2, N, 4] = v
        with pytest.raises(ValueError):
            s._check_pose_scale(B, a)


def test_schedule_without_weights_needs_a_diagonal_problem():
    s = _fake_solver()
    q, p, r = s._own_weights(3)
    np.testing.assert_array_equal(q, np.full((3, 12), 2.0))
    np.testing.assert_array_equal(p, np.full((3, 12), 3.0))
    np.testing.assert_array_equal(r, np.full((3, 6), 0.5))
    for name in ("Q", "P"):
        W = np.eye(12)
        W[1, 7] = W[7, 1] = 0.1
        with pytest.raises(ValueError, match="%s is not diagonal" % name):
            _fake_solver(**{name: W})._own_weights(3)


def test_schedule_path_errors():
    s = _fake_solver()
    s.max_batch, s._sched_next = 8, None
    for bad in (np.ones((3, 1, 6)), np.ones((3, 9, 5)), np.ones((9, 9, 6)), -np.ones((3, 9, 6)), np.full((3, 9, 6), np.nan)):
        with pytest.raises(ValueError):
            s.set_pose_schedule_windows(bad, 0)
    with pytest.raises(ValueError):
        s.set_pose_schedule_windows(np.ones((3, 9, 6)), -1)
    s.set_pose_schedule_windows(None, 0)
    assert s._sched_next is None


def test_gates_workload_is_seeded_and_scaled_at_the_gates():
    B, N, G = 7, 40, 3
    a = workloads.se3_gates(B, N=N, gates=G, gate_gain=32.0)
    b = workloads.se3_gates(B, N=N, gates=G, gate_gain=32.0)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)
    c = workloads.se3_gates(B, N=N, gates=G, gate_gain=32.0, seed=workloads.SEED + 3)
    assert not np.array_equal(a[1], c[1]) and not np.array_equal(a[5], c[5])
    prob, q, xi, us, s, knots = a
    assert s.shape == (B, N + 1, 6) and knots.shape == (B, G) and us.shape == (B, N, 6)
    np.testing.assert_array_equal(knots[0], workloads.gate_knots(N, G))
    np.testing.assert_array_equal(knots[0], [10, 20, 30])
    assert knots.min() >= 1 and knots.max() <= N - 1 and len({tuple(k) for k in knots}) > 1
    for bb in range(B):
        at = np.zeros(N + 1, bool)
        at[knots[bb]] = True
        assert at.sum() == G
        assert np.all(s[bb, at] == 32.0) and np.all(s[bb, ~at] == 1.0)
    # the loose baseline: diagonal weights, the pose block well below se3_tracking's
    base = workloads.se3_tracking(1, N=N)[0]
    assert np.array_equal(prob.Q, np.diag(np.diag(prob.Q))) and np.all(np.diag(prob.Q)[:6] <= 0.01 * np.diag(base.Q)[:6])
    # the defaults the host gate test fixed
    assert workloads.se3_gates.__defaults__ == (200, 3, 64.0, workloads.SEED)
    with pytest.raises(ValueError):
        workloads.se3_gates(2, N=4, gates=4)


def test_window_rule_is_mpc_window_index():
    B, T, N = 5, 9, 4
    path = distinct_schedule(B, T)
    t0 = np.array([0, 3, 7, 9, 1])
    for t in (0, 2, 6, 30):
        w = gather_windows(path, t0, t, N)
        idx = mpc_window_index(t0, t, N, T)
        for b in range(B):
            for i in range(N + 1):
                k = min(int(t0[b]) + t + i, T)
                assert idx[b, i] == k
                np.testing.assert_array_equal(w[b, i], path[b, k])
    np.testing.assert_array_equal(gather_windows(path, None, 1, N), path[:, 1:N + 2])
    np.testing.assert_array_equal(gather_windows(path, None, 8, N)[:, 1:], np.broadcast_to(path[:, T:T + 1], (B, N, 6)))  # the clamp


def test_per_knot_restatement_is_the_oracle_under_a_constant_schedule():
    """knot_ops / lin_scheduled / restate_value_scheduled, the reference side of the GPU tests: with s constant along the
    horizon they are the oracle's linearisation and tests/restate.py::restate_value on the problem weighted s (.) Q, s (.) P;
    with a schedule that varies, knot i's terms are those of s_i."""
    N = 6
    prob = workloads.se3_tracking(1, N=N, R_scale=1e-3)[0]
    rng = np.random.default_rng(2)
    xs_q, xs_xi = near(prob.q_ref, prob.xi_ref, rng)
    us = rng.normal(size=(N, 6))
    c = np.array([1.5, 0.5, 2.0, 3.0, 0.25, 1.0])
    ops = knot_ops(prob, np.tile(c, (N + 1, 1)))
    opc = op_of(prob, Q=pose_scaled(prob.Q, c), P=pose_scaled(prob.P, c))
    o = ob.lin_backward(opc, xs_q, xs_xi, us, ms=True)
    J, lx, lxx = lin_scheduled(ops, xs_q, xs_xi, us)
    np.testing.assert_array_equal(lx, o["Lx"])
    np.testing.assert_array_equal(lxx, o["Lxx"])
    assert J == pytest.approx(o["J"], rel=1e-14)
    K = rng.normal(size=(N, 6, 12)) * 0.1
    for a, b in zip(restate_value_scheduled(ops, xs_q, xs_xi, us, K), restate_value(opc, xs_q, xs_xi, us, K)):
        np.testing.assert_array_equal(a, b)
    s = distinct_schedule(1, N)[0]
    _, lx, lxx = lin_scheduled(knot_ops(prob, s), xs_q, xs_xi, us)
    for i in range(N + 1):
        oi = ob.lin_backward(op_of(prob, Q=pose_scaled(prob.Q, s[i]), P=pose_scaled(prob.P, s[i])), xs_q, xs_xi, us, ms=True)
        np.testing.assert_array_equal(lx[i], oi["Lx"][i])
        np.testing.assert_array_equal(lxx[i], oi["Lxx"][i])
    assert not np.array_equal(lx[2], o["Lx"][2])


def test_gates_are_passed_more_tightly_with_the_schedule():
    """workloads.se3_gates at B = 1, N = 20 on the mirror's host generic path (ScheduledCost), eight iterations of multiple
    shooting (the solve has converged by then): the pose error at every gate knot is smaller with the schedule than without
    (the defaults: gate_gain 64 on pose weights a hundredth of se3_tracking's)."""
    N = 20
    prob, q, xi, us, s, knots = workloads.se3_gates(1, N=N)
    kw = dict(mode="ms", n_iterations=8)
    err = {}
    for name, sc in (("schedule", s[0]), ("plain", np.ones((N + 1, 6)))):
        J, _, xs = host_scheduled_solve(prob, knot_ops(prob, sc), q[0], xi[0], us[0], kw)
        assert len(J) == 8 and np.all(np.isfinite(J))
        err[name] = np.array([np.linalg.norm(ob.rminus(xs[i][0], prob.q_ref[i])) for i in range(N + 1)])
    print("gate knots", knots[0], "with", err["schedule"][knots[0]], "without", err["plain"][knots[0]])
    assert len(knots[0]) == 3
    for g in knots[0]:
        assert err["schedule"][g] < err["plain"][g], g
