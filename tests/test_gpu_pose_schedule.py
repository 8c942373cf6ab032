"""Pose schedules (tolg_set_pose_schedule, pose_scale=): a factor s[b, i, k] on the pose weights that knot i of trajectory b reads.

1. ones are nothing: pose_scale = 1 gives the bits of the run with per-trajectory weights alone;
2. a constant factor is a weight: s = 4 gives the bits of the weights times 4, a per-trajectory constant the weighted run;
3. per-knot linearisation: l_x, l_xx of every knot against ob.cost on that knot's own problem, F_x untouched;
4. solve parity with the mirror's host generic path on a cost plugin that dispatches on the knot;
5. windows gathered on the device are the host-gathered ones; mpc(pose_scale_path=) is the loop of public calls;
6. the held policy: policy_value against the per-knot restatement, policy_rollout's J;
7. the handle's rules through the C ABI, and one case under TOLG_POISON_LDS=1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import mpc_window_index
from tests.schedule import (distinct_schedule, gather_windows, host_scheduled_solve, knot_ops, lin_scheduled,
                            restate_value_scheduled, run_small_scheduled_case, small_scheduled_case, truncated)
from tests.support import (B13, MODES, ZERO, assert_bitwise, bits, broadcast, case_b13, held_policy, host, model_case,
                           moment_inputs, problem_of_kind, random_traj_embedded, rel, rel_nan, same)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bw(prob, B):
    """the problem's own weights, once per trajectory"""
    t = lambda a: np.broadcast_to(np.asarray(a, float), (B,) + np.shape(a)).copy()  # noqa: E731
    return dict(Q=t(prob.Q), P=t(prob.P), R=t(prob.R))


def _pose_times(W, f):
    """W [B, 12, 12] with the pose block's diagonal times f (a scalar or [B])"""
    W = W.copy()
    k = np.arange(6)
    W[:, k, k] = W[:, k, k] * np.reshape(f, (-1, 1))
    return W


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("refs", [False, True], ids=["shared-ref", "pt-ref"])
@pytest.mark.parametrize("case", ["se3", "drone", "so3", "pendulum", "dense"])
def test_ones_are_bitwise_the_weights_alone(case, refs, mode):
    prob, q, xi, us = case_b13(case)
    rk = dict(zip(("q_ref", "xi_ref"), broadcast(prob, B13))) if refs else {}
    kw = MODES[mode]
    r0 = BatchedTrackingILQR(prob, B13).fit_batch(q, xi, us, **rk, **_bw(prob, B13), **kw)
    r1 = BatchedTrackingILQR(prob, B13).fit_batch(q, xi, us, **rk, **_bw(prob, B13), pose_scale=np.ones((B13, prob.N + 1, 6)), **kw)
    torch.cuda.synchronize()
    assert_bitwise(r0, r1, what=case)


def test_ones_one_call_al_and_the_problems_own_weights():
    prob, q, xi, us = case_b13("se3")
    kw = dict(mode="ms", n_iterations=12, **ZERO)
    one = np.ones(prob.N + 1)
    r0 = BatchedTrackingILQR(prob, B13).solve_batch_one_call(q, xi, us, **_bw(prob, B13), **kw)
    r1 = BatchedTrackingILQR(prob, B13).solve_batch_one_call(q, xi, us, **_bw(prob, B13), pose_scale=one, **kw)
    assert_bitwise(r0, r1, what="one call")
    # no Q / P / R: the schedule sits on the problem's own weights, the broadcast-weights run
    r2 = BatchedTrackingILQR(prob, B13).fit_batch(q, xi, us, pose_scale=one, **kw)
    r3 = BatchedTrackingILQR(prob, B13).fit_batch(q, xi, us, **_bw(prob, B13), **kw)
    torch.cuda.synchronize()
    assert_bitwise(r2, r3, what="own weights")
    prob, q, xi, us, lb, ub = workloads.al_tracking(B13, N=200)
    akw = dict(n_al_iters=3, n_ilqr_iters=20)
    a0, i0 = BatchedTrackingILQR(prob, B13).al_fit_batch(q, xi, us, lb, ub, **_bw(prob, B13), **akw)
    a1, i1 = BatchedTrackingILQR(prob, B13).al_fit_batch(q, xi, us, lb, ub, **_bw(prob, B13), pose_scale=np.ones((B13, 201)), **akw)
    torch.cuda.synchronize()
    assert_bitwise(a0, a1, what="al")
    for k in ("lmbd", "Imu", "mu", "max_violation"):
        assert torch.equal(bits(i0[k]), bits(i1[k])), k
    assert i0["outer_iterations"] == i1["outer_iterations"]


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_a_factor_of_four_is_bitwise_the_weights_times_four(mode):
    B = B13
    prob, q, xi, us, Q, P, R, idx, sets = workloads.se3_weight_sweep(B, 3)
    kw = MODES[mode]
    r0 = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us, Q=_pose_times(Q, 4.0), P=_pose_times(P, 4.0), R=R, **kw)
    r1 = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us, Q=Q, P=P, R=R, pose_scale=np.full((B, prob.N + 1, 6), 4.0), **kw)
    plain = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us, Q=Q, P=P, R=R, **kw)
    torch.cuda.synchronize()
    assert_bitwise(r0, r1, what=mode)
    assert not torch.equal(bits(plain.us), bits(r1.us))  # the factor moved the solve


@pytest.mark.parametrize("mode", list(MODES))
def test_a_constant_per_trajectory_is_that_trajectorys_weight(mode):
    """s = 1 + 0.1 b at every knot against the run weighted with Q[:, :6] s, P[:, :6] s: s w is rounded once on both sides, the
    host's product and the kernel's being the same double, so the bounds are test_interleaved_weights_match_the_oracle's at
    the least (J_hist 1e-9, us 1e-6)."""
    B = B13
    prob, q, xi, us, Q, P, R, idx, sets = workloads.se3_weight_sweep(B, 3)
    f = 1.0 + 0.1 * np.arange(B)
    kw = MODES[mode]
    r0 = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us, Q=_pose_times(Q, f), P=_pose_times(P, f), R=R, **kw)
    s = np.broadcast_to(f[:, None, None], (B, prob.N + 1, 6))
    r1 = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us, Q=Q, P=P, R=R, pose_scale=s[:, :, 0], **kw)
    torch.cuda.synchronize()
    assert torch.equal(r0.iters, r1.iters) and torch.equal(r0.status, r1.status)
    for b in range(B):
        n = int(r0.iters[b])
        e_J, e_u = rel_nan(host(r1.J_hist)[b, :n], host(r0.J_hist)[b, :n]), rel_nan(host(r1.us)[b], host(r0.us)[b])
        assert e_J < 1e-9 and e_u < 1e-6, (b, e_J, e_u)


# 3 -------------------------------------------------------------------------------------------------------------------
def _lin_problem(kind, N):
    if kind == "pendulum":
        return truncated(workloads.pendulum_swingup(1)[0], N)
    return problem_of_kind(kind, 1, N)[0]


@pytest.mark.parametrize("ms", [True, False], ids=["ms", "ss"])
@pytest.mark.parametrize("N", [2, 12])
@pytest.mark.parametrize("B", [13, 65])
@pytest.mark.parametrize("kind", ["se3", "drone", "so3", "pendulum"])
def test_linearisation_per_knot(kind, B, N, ms):
    """l_x and the pose block of l_xx of every knot, terminal included (so3 and the pendulum: the terminal l_x keeps Q, scaled
    by s_N), against ob.cost on that knot's problem to 1e-11 (test_linearize_backward_per_trajectory_weights' bound); the cost
    to 1e-12; F_x the bits of the run without a schedule."""
    prob = _lin_problem(kind, N)
    xs_q, xs_xi, us = random_traj_embedded(prob, B, seed=5 + N, spread=0.3)
    if prob.kind == "pendulum3d":  # the embedding's unused coordinates stay at zero, as for so3
        xs_q[..., :3, 3] = prob.q_ref[:, :3, 3]
        xs_xi[..., 3:] = prob.xi_ref[:, 3:]
        us[..., 3:] = 0.0
    s = distinct_schedule(B, N)
    solver = BatchedTrackingILQR(prob, B)
    r0 = solver.linearize_backward(xs_q, xs_xi, us, ms=ms, **_bw(prob, B))
    Fx0 = r0["Fx"].clone()
    r = solver.linearize_backward(xs_q, xs_xi, us, ms=ms, pose_scale=s)
    torch.cuda.synchronize()
    assert torch.equal(bits(Fx0), bits(r["Fx"]))
    assert not torch.equal(bits(r0["lx"]), bits(r["lx"]))
    worst = dict(lx=0.0, lxx=0.0, J=0.0)
    for b in range(B):
        J, lx, lxx = lin_scheduled(knot_ops(prob, s[b]), xs_q[b], xs_xi[b], us[b])
        worst["lx"] = max(worst["lx"], rel(host(r["lx"])[b], lx))
        worst["lxx"] = max(worst["lxx"], rel(host(r["lxx11"])[b], lxx[:, :6, :6]))
        worst["J"] = max(worst["J"], abs(float(r["J"][b]) / J - 1))
    print("%s B=%d N=%d ms=%d" % (kind, B, N, ms), worst)
    assert worst["lx"] < 1e-11 and worst["lxx"] < 1e-11 and worst["J"] < 1e-12


# 4 -------------------------------------------------------------------------------------------------------------------
SOLVES = [dict(mode="ms", n_iterations=10), dict(mode="ss", n_iterations=10), dict(mode="ms", n_iterations=10, line_search=True),
          dict(mode="ms", n_iterations=10, rollout="linear")]


@pytest.mark.parametrize("kw", SOLVES, ids=["ms", "ss", "merit", "linear"])
@pytest.mark.parametrize("kind", ["se3", "drone"])
def test_solve_parity_with_the_host_generic_path(kind, kw):
    B, N = 3, 12
    prob, q, xi, us0 = problem_of_kind(kind, B, N)
    s = distinct_schedule(B, N)
    r = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us0, pose_scale=s, check_every=0, **ZERO, **kw)
    torch.cuda.synchronize()
    for b in range(B):
        J, us, _ = host_scheduled_solve(prob, knot_ops(prob, s[b]), q[b], xi[b], us0[b], kw)
        n = int(r.iters[b])
        assert n == len(J), (b, n, len(J))
        # (a search may end a converged solve with "no descent": the host's last step then gained nothing either, and both
        # stopped at the same iteration)
        assert int(r.status[b]) == _capi.ST_OK or (int(r.status[b]) == _capi.ST_NODESCENT and
                                                   J[-1] >= J[-2] * (1 - 1e-12)), (b, int(r.status[b]), J[-2:])
        e_J =np.abs(host(r.J_hist)[b, :n] / J - 1).max()
        e_u = np.abs(host(r.us)[b] - us).max() / max(1.0, np.abs(us).max())
        print(kind, kw, b, "J_hist %.2e us %.2e" % (e_J, e_u))
        assert e_J < 1e-9 and e_u < 1e-6, (b, e_J, e_u)  # tests/test_gpu_obstacles.py:130-132


def test_al_solve_parity_with_a_sphere_and_a_schedule():
    """al_fit_batch's first outer round (lambda = 0, I_mu = mu0) with one keep-out sphere per trajectory and a schedule, against
    host_solve's construction around ScheduledCost."""
    B, N, mu0 = 3, 12, 5.0
    prob, q, xi, us0 = workloads.se3_tracking(B, N=N, R_scale=1e-3)
    obs = np.empty((B, 1, 4))
    to_ref = prob.q_ref[N][:3, 3][None] - q[:, :3, 3]  # a sphere each trajectory starts inside, on its way to the reference
    obs[:, 0, :3] = q[:, :3, 3] + (0.2 + 0.05 * np.arange(B))[:, None] * to_ref / np.linalg.norm(to_ref, axis=1, keepdims=True)
    obs[:, 0, 3] = 0.5
    s = distinct_schedule(B, N)
    kw = dict(mode="ms", n_iterations=10)
    r, info = BatchedTrackingILQR(prob, B).al_fit_batch(q, xi, us0, obstacles=obs, n_al_iters=1, n_ilqr_iters=10, mu0=mu0,
                                                        pose_scale=s, **ZERO)
    torch.cuda.synchronize()
    lam, imu = np.zeros((N + 1, 1)), np.full((N + 1, 1), mu0)
    active = 0
    for b in range(B):
        J, us, xs = host_scheduled_solve(prob, knot_ops(prob, s[b]), q[b], xi[b], us0[b], kw, obs=obs[b], lam=lam, imu=imu)
        n = int(r.iters[b])
        assert n == len(J) and int(r.status[b]) == 0
        assert np.abs(host(r.J_hist)[b, :n] / J - 1).max() < 1e-9, b
        assert np.abs(host(r.us)[b] - us).max() < 1e-6 * max(1.0, np.abs(us).max()), b
        t = np.array([x[0][:3, 3] for x in xs])
        active += int((np.linalg.norm(t - obs[b, 0, :3], axis=1) < obs[b, 0, 3]).any())
    assert active >= 1  # the sphere's terms were live somewhere


# 5 -------------------------------------------------------------------------------------------------------------------
def test_windows_are_the_host_gathered_schedule():
    B, N, T = 5, 8, 11
    prob = workloads.se3_tracking(1, N=N, R_scale=1e-3)[0]
    xs_q, xs_xi, us = random_traj_embedded(prob, B, seed=9, spread=0.3)
    path = distinct_schedule(B, T)
    t0 = np.array([0, 3, 7, 11, 1], dtype=np.int32)
    s = BatchedTrackingILQR(prob, B)
    # (t, t0, knots past T): none of a trajectory's, some of them, with t0 = NULL, nearly all
    for t, phase, past in ((0, t0[::-1] // 4, 0), (2, t0, 17), (6, None, 3 * B), (9, t0, 40)):
        want = gather_windows(path, phase, t, N)
        raw = (np.zeros(B, int) if phase is None else phase)[:, None] + t + np.arange(N + 1)[None, :]
        assert int((raw > T).sum()) == past
        s.set_pose_schedule_windows(path, t, t0=phase)
        a = s.linearize_backward(xs_q, xs_xi, us, ms=True)
        a = {k: v.clone() for k, v in a.items()}
        b = s.linearize_backward(xs_q, xs_xi, us, ms=True, pose_scale=want)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), (t, k)
        c = s.linearize_backward(xs_q, xs_xi, us, ms=True)  # the staged windows were that one call's
        d = BatchedTrackingILQR(prob, B).linearize_backward(xs_q, xs_xi, us, ms=True)
        torch.cuda.synchronize()
        assert torch.equal(bits(c["lx"]), bits(d["lx"])) and not torch.equal(bits(c["lx"]), bits(a["lx"]))


def test_mpc_with_a_schedule_path_is_the_loop_of_public_calls():
    B, N, steps, K0, K = 5, 8, 3, 6, 3
    prob, q, xi, pq, px, t0, noise = workloads.se3_mpc(B, steps, N=N, sigma_noise=0.02, seed=21)
    T = pq.shape[1] - 1
    path = distinct_schedule(B, T + 2)  # a schedule path of its own length
    s = BatchedTrackingILQR(prob, B)
    seen = []
    r = s.mpc(q, xi, pq, px, steps, t0=t0, first_iters=K0, iters_per_step=K, warm="controls", noise=noise, check_every=0, **ZERO,
              pose_scale_path=path,
              on_step=lambda t, out: seen.append({k: getattr(out, k).clone() for k in ("xs_q", "xs_xi", "us", "J_hist")}))
    torch.cuda.synchronize()
    # afterwards the handle holds no schedule and no weights: the shared solve of a fresh handle
    kw = dict(mode="ms", n_iterations=4, **ZERO)
    assert_bitwise(s.fit_batch(q, xi, None, **kw), BatchedTrackingILQR(prob, B).fit_batch(q, xi, None, **kw), what="after mpc")
    # the same loop, spelled out
    p = BatchedTrackingILQR(prob, B)
    J = torch.zeros(B, dtype=torch.float64, device=p.device)
    x_q, x_xi, us = q, xi, None
    rows = np.arange(B)[:, None]
    for t in range(steps):
        idx = mpc_window_index(t0, t, N, T)
        p.set_pose_schedule_windows(path, t, t0=t0)
        out = p.fit_batch(x_q, x_xi, us, mode="ms", n_iterations=K0 if t == 0 else K, check_every=0, **ZERO,
                          q_ref=pq[rows, idx], xi_ref=px[rows, idx])
        for k, v in seen[t].items():
            assert same(v, getattr(out, k)), (t, k)
        a = p.mpc_advance(noise[:, t], J_cl=J)
        assert same(a["u"], r.us[:, t]) and same(a["x_next_q"], r.xs_q[:, t + 1]) and same(a["x_next_xi"], r.xs_xi[:, t + 1])
        x_q, x_xi, us = a["x_next_q"], a["x_next_xi"], a["us"]
    assert same(J, r.J)
    # and the schedule mattered
    r0 = BatchedTrackingILQR(prob, B).mpc(q, xi, pq, px, steps, t0=t0, first_iters=K0, iters_per_step=K, warm="controls",
                                          noise=noise, check_every=0, **ZERO)
    assert not same(r0.us, r.us)


# 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["se3", "drone", "so3"])
def test_policy_value_against_the_per_knot_restatement(model):
    """tests/test_gpu_value.py::_check_parity with knot i's cost from op_i: every figure below its 1e-9."""
    B, N = 5, 12
    prob, q, xi, us = model_case(model, B, N=N)
    s = distinct_schedule(B, N)
    solver = BatchedTrackingILQR(prob, B)
    r = held_policy(solver, q, xi, us, "ms", pose_scale=s)
    S0, W, S0r, Wr = moment_inputs(prob, B)
    v = solver.policy_value(S0, W, full=True)
    K = host(solver.gains()["K"])
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    worst = 0.0
    for b in range(B):
        P, p, diag_P, price, excess = restate_value_scheduled(knot_ops(prob, s[b]), xq[b], xx[b], uu[b], K[b], S0r[b], Wr[b])
        scale = np.abs(P).max()
        errs = dict(P=np.abs(host(v.P)[b] - P).max() / scale, p=np.abs(host(v.p)[b] - p).max() / scale,
                    diag_P=np.abs(host(v.diag_P)[b] - diag_P).max() / scale,
                    price=np.abs(host(v.price)[b] - price).max() / abs(excess), excess=abs(host(v.excess)[b] - excess) / abs(excess))
        for k, e in errs.items():
            assert e < 1e-9, (model, b, k, e)
        worst = max(worst, *errs.values())
    print("%s value parity %.2e" % (model, worst))
    # against the unscheduled restatement the figures are far off: the kernel read the schedule
    plain = restate_value_scheduled(knot_ops(prob, np.ones((N + 1, 6))), xq[0], xx[0], uu[0], K[0], S0r[0], Wr[0])[0]
    assert np.abs(host(v.P)[0] - plain).max() / np.abs(plain).max() > 1e-3


@pytest.mark.parametrize("model", ["se3", "so3"])
def test_zero_perturbation_rollout_reports_the_scheduled_cost(model):
    """A single-shooting solve under a schedule, then policy_rollout with no perturbation: the solve's own trajectory, and
    its J the solve's last accepted cost to 1e-12 (test_zero_perturbation_reproduces_the_single_shooting_solution's bound)."""
    B, N = 5, 12
    prob, q, xi, us = model_case(model, B, N=N)
    s = distinct_schedule(B, N)
    solver = BatchedTrackingILQR(prob, B)
    r = solver.fit_batch(q, xi, us, mode="ss", n_iterations=25, pose_scale=s)
    p = solver.policy_rollout(S=1)
    its, st, Jh = host(r.iters), host(r.status), host(r.J_hist)
    n = 0
    for b in range(B):
        if its[b] > 0 and st[b] == _capi.ST_OK:
            assert abs(host(p.J)[b, 0] / Jh[b, its[b] - 1] - 1) < 1e-12, b
            n += 1
    assert n >= 3
    # the unscheduled cost of the same trajectory is another number
    J1 = np.array([sum(ob.cost(knot_ops(prob, np.ones((N + 1, 6)))[0], host(r.xs_q)[b, i], host(r.xs_xi)[b, i],
                               host(r.us)[b, i] if i < N else None, i, terminal=(i == N))[0] for i in range(N + 1)) for b in range(B)])
    # (member 0 starts on the reference: its pose error, and with it the schedule's share of its cost, is next to nothing)
    assert np.all(np.abs(host(p.J)[1:, 0] / J1[1:] - 1) > 1e-3)


# 7 -------------------------------------------------------------------------------------------------------------------
def Pt(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def test_handle_rules():
    B, N, E = 3, 4, -1
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, 4)
    lib, h, st = s.lib, s._h, s._stream()
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=s.device)  # noqa: E731
    qd, pd, rd = (dev(np.broadcast_to(np.diag(W), (B, W.shape[0]))) for W in (prob.Q, prob.P, prob.R))
    wbytes, sbytes = int(lib.tolg_weights_bytes(C.byref(s._p), 4)), int(lib.tolg_pose_schedule_bytes(C.byref(s._p), 4))
    assert sbytes == (N + 1) * 6 * 4 * 8
    wbuf, sbuf = torch.zeros(wbytes // 8, device=s.device, dtype=torch.float64), torch.zeros(sbytes // 8, device=s.device, dtype=torch.float64)
    sc = dev(distinct_schedule(B, N))
    path = dev(distinct_schedule(B, N + 3))
    attach = lambda b=B, nb=sbytes: lib.tolg_set_pose_schedule(h, b, Pt(sc), Pt(sbuf), C.c_size_t(nb), st)  # noqa: E731
    weights = lambda b=B: lib.tolg_set_weights(h, b, Pt(qd), Pt(pd), Pt(rd), Pt(wbuf), C.c_size_t(wbytes), st)  # noqa: E731
    kw = dict(mode="ms", n_iterations=2, **ZERO)

    def fit(b=B):  # on what the handle holds: the Python layer sets nothing of its own
        r = s.fit_batch(q[:b], xi[:b], us[:b], **kw)
        torch.cuda.synchronize()
        return r

    want = BatchedTrackingILQR(prob, 4).fit_batch(q, xi, us, pose_scale=distinct_schedule(B, N), **kw)
    shared = BatchedTrackingILQR(prob, 4).fit_batch(q, xi, us, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(bits(want.us), bits(shared.us))
    # without held weights; a detach of nothing is fine
    assert attach() == E
    assert lib.tolg_set_pose_schedule(h, 0, None, None, 0, st) == 0
    assert lib.tolg_set_pose_schedule_windows(h, B, Pt(path), N + 3, None, 0, Pt(sbuf), C.c_size_t(sbytes), st) == E
    # weights for another B, a short or missing buffer, a bad path
    assert weights(2) == 0
    assert attach() == E
    assert weights() == 0
    assert attach(nb=sbytes - 8) == E and attach(b=0) == E and attach(b=5) == E and attach(b=2) == E
    assert lib.tolg_set_pose_schedule(h, B, Pt(sc), None, C.c_size_t(sbytes), st) == E
    for args in ((None, N + 3, None, 0), (Pt(path), 0, None, 0), (Pt(path), N + 3, None, -1)):
        assert lib.tolg_set_pose_schedule_windows(h, B, *args, Pt(sbuf), C.c_size_t(sbytes), st) == E
    assert_bitwise(fit(), shared, what="weights alone")
    assert attach() == 0
    assert_bitwise(fit(), want, what="attached")
    # the one-batch rule: weights for another B are refused while the schedule is held
    assert weights(2) == E
    # the windows form packs the same bits from a path whose window at t = 0 is the schedule
    sbuf_knots = sbuf.clone()
    assert lib.tolg_set_pose_schedule_windows(h, B, Pt(path), N + 3, None, 0, Pt(sbuf), C.c_size_t(sbytes), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(sbuf), bits(sbuf_knots))
    # in flight
    x0q, x0xi, u0 = dev(q.reshape(B, 16)), dev(xi), dev(us)
    opt = _capi.Options(_capi.MODE_MS, 2, 0, 0, 0.0, 0.0, 1e10, _capi.SCHED_AUTO, 0)
    nul = C.c_void_p(0)
    assert lib.tolg_solve_begin(h, C.byref(opt), B, Pt(x0q), Pt(x0xi), Pt(u0), *([nul] * 5), st) == 0
    assert attach() == E and lib.tolg_set_pose_schedule(h, 0, None, None, 0, st) == E
    assert lib.tolg_set_pose_schedule_windows(h, B, Pt(path), N + 3, None, 0, Pt(sbuf), C.c_size_t(sbytes), st) == E
    assert lib.tolg_solve_iterate(h, 2, st) == 0
    out = [torch.empty(B, N + 1, 16, device=s.device, dtype=torch.float64), torch.empty(B, N + 1, 6, device=s.device, dtype=torch.float64),
           torch.empty(B, N, 6, device=s.device, dtype=torch.float64)]
    ints = [torch.empty(B, dtype=torch.int32, device=s.device) for _ in range(3)]
    assert lib.tolg_solve_end(h, *[Pt(t) for t in out + ints], st) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(out[2]), bits(want.us))
    # detaching the schedule leaves the weights; detaching the weights detaches the schedule
    assert lib.tolg_set_pose_schedule(h, 0, None, None, 0, st) == 0
    assert_bitwise(fit(), shared, what="schedule detached")
    assert attach() == 0
    assert lib.tolg_set_weights(h, 0, None, None, None, None, 0, st) == 0
    assert_bitwise(fit(), shared, what="weights detached")
    assert weights() == 0
    assert_bitwise(fit(), shared, what="weights again: no schedule came back")
    assert weights(2) == 0 and weights() == 0  # nothing of the dropped schedule holds the batch
    # re-attaching after a detach
    assert attach() == 0
    assert_bitwise(fit(), want, what="re-attached")
    s.clear_per_trajectory()
    assert_bitwise(fit(), shared, what="cleared")


def test_a_scheduled_solve_under_poisoned_lds():
    """TOLG_POISON_LDS is read once per process: the small scheduled solve and its policy_value in a child process with the
    variable set give the bits of this process."""
    import tempfile
    kw = dict(mode="ms", n_iterations=6, line_search=True)
    with tempfile.TemporaryDirectory() as d:
        here, child = os.path.join(d, "here.npz"), os.path.join(d, "child.npz")
        run_small_scheduled_case(here, **kw)
        env = dict(os.environ, TOLG_POISON_LDS="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        code = "from tests.schedule import run_small_scheduled_case as f; f(%r, **%r)" % (child, kw)
        flags = ["-s"] if sys.flags.no_user_site else []
        out = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-2000:]
        a, b = np.load(here), np.load(child)
        for k in a.files:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.isfinite(a["us"]).all() and small_scheduled_case()[4].shape == (5, 13, 6)
