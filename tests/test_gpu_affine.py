"""rollout = 'linear' taken from the affine recursion (k_expected_change_ring<STORE> + k_ls_eval_affine / k_affine_commit,
TOLG_SCHED_AUTO) against the statement-form rollouts (k_rollout / k_rollout_ls / k_rollout_eval_t with LINEAR, the split
schedule) and the CPU oracle.  The reference's linear rollout (traopt_controller.py:2720-2737 MS, :2065-2071 SS) IS that
recursion as long as Log(Exp(v)) = v, i.e. while the rotation part of the predicted deviation stays below pi; trajectories
that leave that range are handed to the statement form inside the same solve -- the last test makes that happen."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import bridge as ob  # noqa: E402  (test infrastructure)
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, workloads  # noqa: E402
from tests.support import oracle_problem, rel  # noqa: E402


def _fit(prob, x0_q, x0_xi, us0, K, mode, line_search, schedule):
    r = BatchedTrackingILQR(prob, x0_q.shape[0]).fit_batch(x0_q, x0_xi, us0, mode=mode, n_iterations=K, tol_grad_norm=0.0,
                                                           tol_d_norm=0.0, line_search=line_search, rollout="linear",
                                                           schedule=schedule)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("kind,mode,line_search,B,N", [
    ("se3", "ms", False, 37, 45), ("se3", "ms", True, 21, 60), ("se3", "ss", False, 19, 33), ("drone", "ms", False, 9, 70),
    ("drone", "ms", True, 13, 41), ("drone", "ss", False, 6, 25), ("se3", "ms", False, 5, 1), ("se3", "ss", False, 4, 2),
    ("se3", "ms", True, 260, 40),   # more undecided trajectories than one workgroup of the evaluation holds
    ("se3_dense", "ms", False, 17, 45), ("se3_dense", "ms", True, 11, 50), ("se3_dense", "ss", False, 9, 33),  # I + H dt from the record
])
def test_affine_equals_statement_form_and_oracle(kind, mode, line_search, B, N):
    prob, x0_q, x0_xi, us0 = (workloads.drone_tracking if kind == "drone" else workloads.se3_tracking)(B, N=N, R_scale=1e-3)
    if kind.endswith("_dense"):  # full inertia blocks (a rotated body frame's inertia): the sweep reads the velocity block from the record
        A = np.array([[0.10, -0.05, 0.02], [0.03, 0.12, -0.04], [-0.02, 0.06, 0.09]])
        Jd = np.array(prob.J, dtype=float).copy()
        Jd[:3, :3] += A @ A.T
        Jd[3:, 3:] += 0.5 * (A @ A.T)
        prob = TrackingProblem("se3", Jd, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
    K = 5
    ra = _fit(prob, x0_q, x0_xi, us0, K, mode, line_search, "auto")
    rs = _fit(prob, x0_q, x0_xi, us0, K, mode, line_search, "split")
    o = ob.fit_batch(oracle_problem(prob), x0_q, x0_xi, us0, mode=mode, max_iter=K, line_search=line_search, rollout="linear")
    # the two GPU forms take the same decisions; against the oracle a search that has converged to rounding level may end on a
    # coin flip (the last step size of the merit search is 1.1^-361 = 1e-15: tests/test_gpu_matrix.py) -- the side that goes on
    # does so without moving the cost
    assert torch.equal(ra.iters, rs.iters) and torch.equal(ra.status, rs.status)
    same = np.ones(B, dtype=bool)
    for b in range(B):
        if ra.iters[b].item() != o["iters"][b] or ra.status[b].item() != o["status"][b]:
            n = int(min(ra.iters[b].item(), o["iters"][b]))
            tail = o["J_hist"][b, max(n - 1, 0): o["iters"][b]]
            assert (line_search or mode == "ss") and np.ptp(tail) <= 1e-10 * abs(tail[0]), (b, ra.iters[b].item(), o["iters"][b])
            same[b] = False
    assert same.sum() >= B - max(1, B // 50)
    n = int(min(o["iters"][same].min(), ra.iters.cpu().numpy()[same].min()))
    for r in (ra, rs):
        assert rel(r.J_hist.cpu().numpy()[same, :n], o["J_hist"][same, :n]) < 1e-9
        assert rel(r.us.cpu().numpy()[same], o["us"][same]) < 1e-6
        assert rel(r.xs_xi.cpu().numpy()[same], o["xs_xi"][same]) < 1e-6
    Ja, Js = ra.J_hist.cpu().numpy(), rs.J_hist.cpu().numpy()   # (NaN = not reached: the same entries on both sides)
    assert np.array_equal(np.isnan(Ja), np.isnan(Js))
    assert rel(np.nan_to_num(Ja), np.nan_to_num(Js)) < 1e-10
    assert rel(ra.us.cpu().numpy(), rs.us.cpu().numpy()) < 1e-8
    if ra.alpha_hist is not None and (line_search or mode == "ss"):
        assert np.array_equal(np.nan_to_num(ra.alpha_hist.cpu().numpy()), np.nan_to_num(rs.alpha_hist.cpu().numpy()))


def test_trajectories_handed_back_take_the_statement_form():
    """Wild initial controls on some members: the linear prediction turns by more than 3 rad somewhere, the recursion hands
    those trajectories back (Log(Exp(v)) != v beyond pi) and the statement-form kernels serve them inside the same stages;
    the tame members of the same batch take the affine path.  Both kinds against the oracle, per trajectory."""
    B, N, K = 24, 40, 3
    prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=N, R_scale=1e-2)
    rng = np.random.default_rng(3)
    us0 = us0.copy()
    wild = np.arange(B) % 3 == 0
    us0[wild] = rng.normal(size=(int(wild.sum()), N, 6)) * 3.0
    x0_xi = x0_xi.copy()
    x0_xi[wild, :3] += rng.normal(size=(int(wild.sum()), 3)) * 4.0
    op = oracle_problem(prob)
    for mode, ls in (("ss", False), ("ms", True)):
        ra = _fit(prob, x0_q, x0_xi, us0, K, mode, ls, "auto")
        rs = _fit(prob, x0_q, x0_xi, us0, K, mode, ls, "split")
        o = ob.fit_batch(op, x0_q, x0_xi, us0, mode=mode, max_iter=K, line_search=ls, rollout="linear")
        checked = 0
        for b in range(B):
            n = int(min(ra.iters[b].item(), rs.iters[b].item(), o["iters"][b]))
            jo = o["J_hist"][b, :n]
            if n == 0 or not np.isfinite(jo).all() or np.abs(jo).max() > 1e12:
                continue
            assert ra.iters[b].item() == rs.iters[b].item() == o["iters"][b], (mode, b)
            assert rel(ra.J_hist[b, :n].cpu().numpy(), jo) < 1e-8, (mode, b)
            assert rel(rs.J_hist[b, :n].cpu().numpy(), jo) < 1e-8, (mode, b)
            checked += 1
        assert checked >= B // 2
