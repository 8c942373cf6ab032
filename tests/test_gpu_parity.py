"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI,
against the CPU oracle and the reference's recorded runs.

Tolerances: BASELINE.json north_star asks <= 1e-6 relative on solved trajectories; the
element-level checks below are far tighter because both sides are fp64."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bridge as ob  # noqa: E402  (test infrastructure)
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, workloads  # noqa: E402
from tests.checks import al_oracle, check_linearize_backward  # noqa: E402
from tests.support import oracle_problem, random_traj, rel  # noqa: E402


@pytest.fixture(scope="module")
def drone(golden_dir):
    g = np.load(os.path.join(golden_dir, "drone_n150_problem.npz"))
    log = json.load(open(os.path.join(golden_dir, "drone_n150_log.json")))
    prob = TrackingProblem("drone", g["J"], float(g["dt"]), g["Q"], g["R"], g["P"], g["q_ref"], g["xi_ref"])
    return g, log, prob


@pytest.mark.parametrize("kind", ["se3", "drone", "rigidbody"])
@pytest.mark.parametrize("ms", [True, False])
def test_linearize_backward_elementwise(kind, ms):
    """K1 + K2 against the oracle's _linearization/_backward_pass on random trajectories
    (B = 5 also exercises the padding to a multiple of 4 trajectories per wavefront)."""
    if kind == "se3":
        prob, *_ = workloads.se3_tracking(1, N=24)
    else:
        prob, *_ = workloads.drone_tracking(1, N=24)
        if kind == "rigidbody":
            prob = TrackingProblem("rigidbody", prob.J, prob.dt, prob.Q, np.eye(6) * 1e-4, prob.P, prob.q_ref, prob.xi_ref)
    B = 5
    xs_q, xs_xi, us = random_traj(prob, B, seed=11)
    check_linearize_backward(prob, xs_q, xs_xi, us, ms)


def test_full_inertia_block_general_path():
    """Non-diagonal I_b / J_v take the general (non diagJ) code path of the dynamics."""
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(3, N=30)
    rng = np.random.default_rng(2)
    A = rng.normal(size=(3, 3)) * 0.2
    J = prob.J.copy()
    J[:3, :3] = np.diag([0.5, 0.7, 0.9]) + A @ A.T
    J[3:, 3:] = 1.3 * np.eye(3)
    prob = TrackingProblem("se3", J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
    solver = BatchedTrackingILQR(prob, 3)
    r = solver.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=8, tol_grad_norm=0.0, tol_d_norm=0.0)
    o = ob.fit_batch(oracle_problem(prob), x0_q, x0_xi, us0, mode="ms", max_iter=8)
    assert rel(r.J_hist.cpu(), o["J_hist"]) < 1e-9
    assert rel(r.us.cpu(), o["us"]) < 1e-6
    # coupling blocks between rotation and translation are rejected, as the reference's G assumes
    Jbad = J.copy(); Jbad[0, 4] = Jbad[4, 0] = 0.01
    with pytest.raises(RuntimeError, match="bad argument"):
        BatchedTrackingILQR(TrackingProblem("se3", Jbad, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref), 3)


def test_regularisation_loop_nonpd_branch():
    """Unpinned by any golden: an indefinite R makes Q_uu non-PD so the
    mu/delta schedule (traopt_controller.py:2977-2991) has to fire; the oracle is the reference."""
    prob, *_ = workloads.se3_tracking(1, N=16)
    R = np.diag([-30.0, 1e-3, 1e-3, -5.0, 1e-3, 1e-3])
    prob = TrackingProblem("se3", prob.J, prob.dt, prob.Q, R, prob.P, prob.q_ref, prob.xi_ref)
    B = 4
    xs_q, xs_xi, us = random_traj(prob, B, seed=5, spread=0.1)
    solver = BatchedTrackingILQR(prob, B)
    r = solver.linearize_backward(xs_q, xs_xi, us, ms=True)
    op = oracle_problem(prob)
    fired = False
    for b in range(B):
        o = ob.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=True)
        fired |= o["mu"] > 1.0
        assert float(r["mu_delta"][b, 0]) == pytest.approx(o["mu"], rel=1e-15)
        assert float(r["mu_delta"][b, 1]) == pytest.approx(o["delta"], rel=1e-15)
        assert rel(r["K"][b].cpu(), o["K"]) < 1e-7
        assert float(r["grad"][b]) == pytest.approx(o["grad"], rel=1e-8)
    assert fired


def test_drone_ms_fit_reproduces_recorded_run(drone):
    """B = 3 copies of the notebook problem: every recorded J / gradient of the 28 MS iterations."""
    g, log, prob = drone
    B = 3
    solver = BatchedTrackingILQR(prob, B)
    x0_q = np.repeat(g["q0"][None], B, 0); x0_xi = np.repeat(g["xi0"][None], B, 0)
    r = solver.fit_batch(x0_q, x0_xi, None, mode="ms", n_iterations=200, tol_grad_norm=1e-12)
    torch.cuda.synchronize()
    its = [it for it in log["ms"]["iterations"] if "J_new" in it]
    J = r.J_hist.cpu().numpy(); G = r.grad_hist.cpu().numpy(); D = r.defect_hist.cpu().numpy()
    for b in range(B):
        assert int(r.iters[b]) == 28 and int(r.converged[b]) == 1 and int(r.status[b]) == 0
        assert D[b, 0] == pytest.approx(its[0]["defect_lin"], rel=1e-12)
        for k, it in enumerate(its):
            assert J[b, k] == pytest.approx(it["J_new"], rel=1e-11)
            assert G[b, k] == pytest.approx(it["grad"], rel=1e-7, abs=2e-14)
            assert D[b, k + 1] < 1e-12
    # identical inputs -> bitwise identical outputs across the batch (no cross-talk, deterministic)
    assert torch.equal(r.us[0], r.us[1]) and torch.equal(r.xs_q[0], r.xs_q[2])
    # final trajectory against the oracle (north_star: <= 1e-6 relative)
    o = ob.fit(oracle_problem(prob), g["q0"], g["xi0"], g["us_init"], mode="ms", max_iter=200, tol_grad=1e-12)
    assert rel(r.us[0].cpu(), o["us"]) < 1e-6
    assert rel(r.xs_q[0].cpu(), o["xs_q"]) < 1e-6
    assert rel(r.xs_xi[0].cpu(), o["xs_xi"]) < 1e-6


def test_se3_batch_matches_oracle_per_trajectory():
    """BASELINE config 3 shape at a size the oracle finishes in seconds: B = 12, N = 200."""
    B = 12
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=200)
    solver = BatchedTrackingILQR(prob, B)
    K = 12
    r = solver.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0)
    o = ob.fit_batch(oracle_problem(prob), x0_q, x0_xi, us0, mode="ms", max_iter=K)
    assert rel(r.J_hist.cpu(), o["J_hist"]) < 1e-9
    assert rel(r.defect_hist.cpu()[:, 0], o["defect_hist"][:, 0]) < 1e-12
    assert rel(r.us.cpu(), o["us"]) < 1e-6
    assert rel(r.xs_q.cpu(), o["xs_q"]) < 1e-6
    assert rel(r.xs_xi.cpu(), o["xs_xi"]) < 1e-6
    assert (r.iters.cpu().numpy() == K).all()


def test_convergence_masks_freeze_finished_trajectories():
    """Per-trajectory convergence: trajectories stop at different iterations and keep their result."""
    B = 8
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=60, R_scale=1e-3)
    solver = BatchedTrackingILQR(prob, B)
    r = solver.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=60, tol_grad_norm=1e-7)
    o = ob.fit_batch(oracle_problem(prob), x0_q, x0_xi, us0, mode="ms", max_iter=60, tol_grad=1e-7, tol_defect=1e-6)
    assert (r.converged.cpu().numpy() == 1).all()
    np.testing.assert_array_equal(r.iters.cpu().numpy(), o["iters"])
    # the closed defects must stay at rounding level for every later iteration (a quaternion
    # double-cover sign slip in Log makes them double per iteration instead)
    D = r.defect_hist.cpu().numpy()
    for b in range(B):
        assert np.nanmax(D[b, 1:]) < 1e-12
    assert rel(r.us.cpu(), o["us"]) < 1e-6


def test_full_size_properties_4096x200():
    """BASELINE metric size (too big for the oracle): size-independent properties."""
    B, N, K = 4096, 200, 4
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=N)
    # plant duplicates and a known small sub-batch
    x0_q[1000] = x0_q[7]; x0_xi[1000] = x0_xi[7]
    x0_q[4095] = x0_q[0]; x0_xi[4095] = x0_xi[0]
    solver = BatchedTrackingILQR(prob, B)
    r1 = solver.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0)
    us1 = r1.us.clone(); J1 = r1.J_hist.clone()
    # determinism: same inputs twice -> bitwise equal (stands in for a race detector)
    r2 = solver.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0)
    assert torch.equal(us1, r2.us) and torch.equal(J1, r2.J_hist)
    # duplicates agree bitwise, wherever they sit in the batch (wave / lane-group position)
    assert torch.equal(us1[1000], us1[7]) and torch.equal(us1[4095], us1[0])
    # batch permutation equivariance
    perm = np.random.default_rng(0).permutation(B)
    r3 = solver.fit_batch(x0_q[perm], x0_xi[perm], us0, mode="ms", n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0)
    assert torch.equal(r3.us, us1[torch.as_tensor(perm, device=us1.device)])
    # a sub-batch solved alone gives the same answer as inside the big batch, and matches the oracle
    sub = [0, 7, 513, 2049]
    rs = BatchedTrackingILQR(prob, len(sub)).fit_batch(x0_q[sub], x0_xi[sub], us0[sub], mode="ms", n_iterations=K,
                                                         tol_grad_norm=0.0, tol_d_norm=0.0)
    assert torch.equal(rs.us, us1[sub])
    o = ob.fit_batch(oracle_problem(prob), x0_q[sub], x0_xi[sub], us0[sub], mode="ms", max_iter=K)
    assert rel(rs.us.cpu(), o["us"]) < 1e-6
    # the MS nonlinear rollout closes the defects to rounding after the first iteration
    D = r1.defect_hist.cpu().numpy()
    assert (D[:, 0] > 1.0).all() and (D[:, 1:K + 1] < 1e-10).all()
    # rotations stay orthonormal
    Rm = r1.xs_q[:, :, :3, :3]
    assert float((Rm.transpose(-1, -2) @ Rm - torch.eye(3, device=Rm.device, dtype=Rm.dtype)).abs().max()) < 1e-13


def test_drone_ss_fit_reproduces_recorded_line_search(drone):
    """Single shooting with the 13-alpha backtracking: the notebook's 9 iterations, including the
    failed line search of iteration 8 (status NODESCENT, every trial cost recorded)."""
    g, log, prob = drone
    B = 2
    solver = BatchedTrackingILQR(prob, B)
    x0_q = np.repeat(g["q0"][None], B, 0); x0_xi = np.repeat(g["xi0"][None], B, 0)
    r = solver.fit_batch(x0_q, x0_xi, None, mode="ss", n_iterations=200, tol_grad_norm=1e-12)
    its = log["ss"]["iterations"]
    J = r.J_hist.cpu().numpy(); G = r.grad_hist.cpu().numpy(); A = r.alpha_hist.cpu().numpy()
    for b in range(B):
        assert int(r.iters[b]) == 9 and int(r.status[b]) == 2 and int(r.converged[b]) == 0
        for k, it in enumerate(its):
            assert G[b, k] == pytest.approx(it["grad"], rel=1e-9)
            assert J[b, k] == pytest.approx(it["cb_J"], rel=1e-11)
            assert A[b, k] == pytest.approx(it["cb_alpha"], rel=1e-14)
    o = ob.fit(oracle_problem(prob), g["q0"], g["xi0"], g["us_init"], mode="ss", max_iter=200, tol_grad=1e-12)
    assert rel(r.us[0].cpu(), o["us"]) < 1e-6 and rel(r.xs_q[0].cpu(), o["xs_q"]) < 1e-6


@pytest.mark.parametrize("mode,line_search,rollout", [("ss", False, "nonlinear"), ("ss", False, "linear"),
                                                      ("ms", True, "nonlinear"), ("ms", False, "linear"),
                                                      ("ms", True, "linear")])
def test_line_search_and_linear_rollout_variants_match_oracle(mode, line_search, rollout):
    """Branches no recorded run exercises: the oracle is the reference."""
    B, K = 6, 10
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=50, R_scale=1e-3)
    solver = BatchedTrackingILQR(prob, B)
    r = solver.fit_batch(x0_q, x0_xi, us0, mode=mode, n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0,
                         line_search=line_search, rollout=rollout)
    o = ob.fit_batch(oracle_problem(prob), x0_q, x0_xi, us0, mode=mode, max_iter=K, line_search=line_search,
                     rollout=rollout)
    it_g = r.iters.cpu().numpy()
    np.testing.assert_array_equal(it_g, o["iters"])
    np.testing.assert_array_equal(r.status.cpu().numpy(), o["status"])
    Jg = r.J_hist.cpu().numpy()
    for b in range(B):
        n = it_g[b]
        assert rel(Jg[b, :n], o["J_hist"][b, :n]) < 1e-8
    assert rel(r.us.cpu(), o["us"]) < 1e-6
    assert rel(r.xs_xi.cpu(), o["xs_xi"]) < 1e-6


def test_augmented_lagrangian_input_box_matches_restated_outer_loop():
    """BASELINE config 4 shape (SE3 AL-DDP multiple shooting with input box constraints), small."""
    from scipy.linalg import expm
    N, dt, B = 40, 0.01, 3
    xi_c = np.array([0.0, 0.0, 1.0, 2.0, 0.0, 0.2])
    hat = np.zeros((4, 4)); hat[:3, :3] = [[0, -1.0, 0], [1.0, 0, 0], [0, 0, 0]]; hat[:3, 3] = xi_c[3:]
    q_ref = np.empty((N + 1, 4, 4)); q_ref[0] = np.eye(4)
    for i in range(N):
        q_ref[i + 1] = q_ref[i] @ expm(hat * dt)
    xi_ref = np.repeat(xi_c[None], N + 1, 0)
    Q = np.diag([10.0, 10, 10, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    prob = TrackingProblem("se3", np.diag([0.5, 0.7, 0.9, 1, 1, 1.0]), dt, Q, np.eye(6) * 1e-3, 10 * Q, q_ref, xi_ref)
    q0 = np.eye(4); q0[:3, 3] = [-0.3, -0.3, -0.1]
    xi0 = np.array([0, 0, 0.1, 2.0, 0, 0.2])
    x0_q, x0_xi = workloads.perturbed_batch(q0, xi0, B, 0.1 * np.ones(6), 0.05, seed=3)
    us0 = np.zeros((B, N, 6))
    lb = -4.0 * np.ones(6); ub = 4.0 * np.ones(6)
    solver = BatchedTrackingILQR(prob, B)
    # the unconstrained solution must violate the box, otherwise the test is vacuous
    free = solver.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=60)
    assert float(free.us.abs().max()) > 6.0
    res, info = solver.al_fit_batch(x0_q, x0_xi, us0, lb, ub, n_al_iters=8, n_ilqr_iters=60, tol_constr=1e-2)
    assert int(info["al_converged"].sum()) == B
    assert float(res.us.max()) < 4.0 + 1e-2 and float(res.us.min()) > -4.0 - 1e-2
    for b in range(B):
        o, lam, imu, mu, n_outer = al_oracle(prob, x0_q[b], x0_xi[b], us0[b], lb, ub, 8, 60, 1e-2)
        assert rel(res.us[b].cpu(), o["us"]) < 1e-6
        assert rel(res.xs_xi[b].cpu(), o["xs_xi"]) < 1e-6
        assert rel(info["lmbd"][b].cpu(), lam) < 1e-6
        assert float(info["mu"][b]) == pytest.approx(mu)
        np.testing.assert_array_equal(info["Imu"][b].cpu().numpy() == 0.0, imu == 0.0)


# ---------------------------------------------------------------------------------------------------
# SO(3) (BASELINE config 2): the reference's recorded run of baseline_SO3.ipynb cell 28
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def so3(golden_dir):
    from trajectory_optimization_matrix_lie_groups_amd.solver import embed_so3
    g = np.load(os.path.join(golden_dir, "so3_n249_problem.npz"))
    log = json.load(open(os.path.join(golden_dir, "so3_n249_log.json")))
    prob = embed_so3(g["J"], float(g["dt"]), g["Q"], g["R"], g["P"], g["q_ref"], g["xi_ref"])
    return g, log, prob


def test_so3_ss_fit_reproduces_recorded_run(so3):
    g, log, prob = so3
    q0, xi0 = ob.embed_so3_state(g["q0"], g["xi0"])
    solver = BatchedTrackingILQR(prob, 2)
    r = solver.fit_batch(np.stack([q0, q0]), np.stack([xi0, xi0]), None, mode="ss", n_iterations=100, tol_grad_norm=1e-12)
    its = log["ss"]["iterations"]
    J = r.J_hist.cpu().numpy(); G = r.grad_hist.cpu().numpy(); A = r.alpha_hist.cpu().numpy()
    assert int(r.iters[0]) == 100 and int(r.status[0]) == 0
    for k, it in enumerate(its):
        assert J[0, k] == pytest.approx(it["cb_J"], rel=1e-11)
        assert G[0, k] == pytest.approx(it["grad"], rel=1e-7)
        assert A[0, k] == pytest.approx(it["cb_alpha"])
    # unused SE(3) coordinates stay exactly zero; both copies identical
    assert float(r.xs_q[:, :, :3, 3].abs().max()) == 0.0 and float(r.xs_xi[:, :, 3:].abs().max()) == 0.0
    assert float(r.us[:, :, 3:].abs().max()) == 0.0 and torch.equal(r.us[0], r.us[1])
    o = ob.fit(ob.embed_so3_problem(g["J"], float(g["dt"]), g["Q"], g["R"], g["P"], g["q_ref"], g["xi_ref"]), q0, xi0,
               np.zeros((249, 6)), mode="ss", max_iter=100, tol_grad=1e-12)
    assert rel(r.us[0].cpu(), o["us"]) < 1e-6 and rel(r.xs_q[0].cpu(), o["xs_q"]) < 1e-6


def test_so3_ms_merit_search_reproduces_recorded_run(so3):
    """Iterations 0..10 of the recorded MS run with line_search=True (later ones are decided by rounding,
    see tests/test_oracle_golden.py)."""
    g, log, prob = so3
    q0, xi0 = ob.embed_so3_state(g["q0"], g["xi0"])
    solver = BatchedTrackingILQR(prob, 1)
    r = solver.fit_batch(q0[None], xi0[None], None, mode="ms", n_iterations=11, tol_grad_norm=1e-12, line_search=True)
    its = [it for it in log["ms"]["iterations"] if "cb_J" in it]
    J = r.J_hist.cpu().numpy(); G = r.grad_hist.cpu().numpy(); A = r.alpha_hist.cpu().numpy(); D = r.defect_hist.cpu().numpy()
    assert D[0, 0] == pytest.approx(its[0]["defect_lin"], rel=1e-12)
    for k in range(11):
        assert J[0, k] == pytest.approx(its[k]["cb_J"], rel=1e-12)
        assert G[0, k] == pytest.approx(its[k]["grad"], rel=1e-5)
        assert A[0, k] == 1.0 and D[0, k + 1] < 1e-12


def test_so3_linearisation_matches_oracle(so3):
    g, log, prob = so3
    op = ob.embed_so3_problem(g["J"], float(g["dt"]), g["Q"], g["R"], 10 * g["Q"], g["q_ref"], g["xi_ref"])
    from trajectory_optimization_matrix_lie_groups_amd.solver import embed_so3
    prob10 = embed_so3(g["J"], float(g["dt"]), g["Q"], g["R"], 10 * g["Q"], g["q_ref"], g["xi_ref"])  # P != Q: quirk Q3 visible
    rng = np.random.default_rng(8)
    N = 249
    xs_q = np.tile(np.eye(4), (1, N + 1, 1, 1)); xs_xi = np.zeros((1, N + 1, 6)); us = np.zeros((1, N, 6))
    for i in range(N + 1):
        xs_q[0, i, :3, :3] = g["q_ref"][i] @ ob.se3_exp(np.r_[rng.normal(size=3) * 0.3, 0, 0, 0])[:3, :3]
        xs_xi[0, i, :3] = g["xi_ref"][i] + rng.normal(size=3) * 0.3
    us[0, :, :3] = rng.normal(size=(N, 3))
    solver = BatchedTrackingILQR(prob10, 1)
    for ms in (True, False):
        r = solver.linearize_backward(xs_q, xs_xi, us, ms=ms)
        o = ob.lin_backward(op, xs_q[0], xs_xi[0], us[0], ms=ms)
        assert rel(r["Fx"][0].cpu(), o["Fx"]) < 1e-12
        assert rel(r["lx"][0].cpu(), o["Lx"]) < 1e-11            # terminal l_x with Q
        assert rel(r["lxx11"][0].cpu(), o["Lxx"][:, :6, :6]) < 1e-11  # terminal l_xx with P
        assert float(r["J"][0]) == pytest.approx(o["J"], rel=1e-12)
        assert float(r["grad"][0]) == pytest.approx(o["grad"], rel=1e-9)
        assert rel(r["K"][0].cpu(), o["K"]) < 1e-8


# ---------------------------------------------------------------------------------------------------
# Edge sizes: one knot, odd horizons, batches that are not a multiple of the 4-trajectory interleave
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 1), (2, 2), (3, 3), (5, 7), (7, 9), (1, 200)])
@pytest.mark.parametrize("mode", ["ms", "ss"])
def test_edge_sizes_match_oracle(B, N, mode):
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=N, R_scale=1e-3)
    solver = BatchedTrackingILQR(prob, B)
    K = 6
    r = solver.fit_batch(x0_q, x0_xi, us0, mode=mode, n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0)
    o = ob.fit_batch(oracle_problem(prob), x0_q, x0_xi, us0, mode=mode, max_iter=K)
    np.testing.assert_array_equal(r.iters.cpu().numpy(), o["iters"])
    np.testing.assert_array_equal(r.status.cpu().numpy(), o["status"])
    for b in range(B):
        n = int(r.iters[b])
        assert rel(r.J_hist[b, :n].cpu(), o["J_hist"][b, :n]) < 1e-8
    assert rel(r.us.cpu(), o["us"]) < 1e-6
    assert np.abs(r.xs_q.cpu().numpy() - o["xs_q"]).max() < 1e-6


def test_c_abi_rejects_bad_arguments():
    """Error behaviour at the boundary: return codes, no exceptions from the library (include/tolg.h)."""
    import ctypes as C
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import _capi
    lib = _capi.load()
    prob, _, _, _ = workloads.se3_tracking(2, N=5)
    p = _capi.Problem()
    p.kind, p.m, p.N, p.dt = 0, 6, 5, prob.dt
    p.J[:] = list(np.asarray(prob.J).reshape(-1)); p.Q[:] = list(prob.Q.reshape(-1)); p.P[:] = list(prob.P.reshape(-1))
    p.R[:] = list(np.asarray(prob.R).reshape(-1))
    dev = torch.device("cuda:0")
    q_ref = torch.as_tensor(prob.q_ref, device=dev).contiguous(); xi_ref = torch.as_tensor(prob.xi_ref, device=dev).contiguous()
    need = lib.tolg_workspace_bytes(C.byref(p), 2)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    h = C.c_void_p()

    def create(pp, nbytes):
        return lib.tolg_create(C.byref(pp), C.c_void_p(q_ref.data_ptr()), C.c_void_p(xi_ref.data_ptr()), 2,
                               C.c_void_p(ws.data_ptr()), nbytes, None, C.byref(h))
    assert create(p, need // 2) == -2                       # TOLG_E_WORKSPACE
    bad = _capi.Problem.from_buffer_copy(p); bad.m = 5
    assert create(bad, need) == -1                          # TOLG_E_ARG: action size does not fit the model
    bad = _capi.Problem.from_buffer_copy(p); bad.kind = 9
    assert create(bad, need) == -1
    bad = _capi.Problem.from_buffer_copy(p); bad.J[1] = 0.3  # off-diagonal inertia blocks are fine ...
    bad.J[3] = 0.1                                           # ... coupling between I_b and J_v is not
    assert create(bad, need) == -1
    bad = _capi.Problem.from_buffer_copy(p)
    for k in range(36):
        bad.J[k] = 0.0
    assert create(bad, need) == -4                          # TOLG_E_SINGULAR
    assert create(p, need) == 0
    assert lib.tolg_solve_iterate(h, 1, None) == -1          # no solve in flight
    lib.tolg_destroy(h)
