"""CPU pins of the large-rotation suite (tests/test_gpu_large_rotation.py): restate_rollout against the oracle's own rollout,
and the case grid's coverage guard, which needs no device."""
import numpy as np
import pytest

from oracle import bridge as ob
from tests.restate import restate_rollout
from tests.support import (MODELS, assert_coverage, knot_states, large_rotation_problem, model_case, op_of, problem_of_kind,
                           r_to_q)


@pytest.mark.parametrize("rollout", ["nonlinear", "linear"])
@pytest.mark.parametrize("mode", ["ms", "ss"])
@pytest.mark.parametrize("kind", ["se3", "drone", "so3"])
def test_restate_rollout_reproduces_one_oracle_iteration(kind, mode, rollout):
    """One accept-always iteration of ob.fit is linearise + sweep + the alpha = 1 rollout: from ob.lin_backward's gains on the
    initial guess restate_rollout gives the iteration's trajectory."""
    N = 12
    prob, x0_q, x0_xi, us0 = problem_of_kind(kind, 3, N)
    op = op_of(prob)
    rng = np.random.default_rng(4)
    for b in range(3):
        us = us0[b] + rng.normal(size=us0[b].shape) * 0.1 * (np.arange(prob.m) < (3 if kind == "so3" else 6))
        q = np.array(prob.q_ref, float).copy(); xi = np.array(prob.xi_ref, float).copy()
        q[0], xi[0] = x0_q[b], x0_xi[b]
        if mode == "ss":  # the open-loop rollout
            for i in range(N):
                q[i + 1], xi[i + 1] = ob.f(op, q[i], xi[i], us[i])
        o = ob.fit(op, x0_q[b], x0_xi[b], us, mode=mode, max_iter=1, tol_grad=0.0, tol_defect=0.0, rollout=rollout)
        g = ob.lin_backward(op, q, xi, us, ms=(mode == "ms"))
        nq, nxi, nu = restate_rollout(op, q, xi, us, g["k"], g["K"], 1.0, mode == "ms", rollout == "linear")
        assert np.abs(nq - o["xs_q"]).max() < 1e-12
        assert np.abs(nxi - o["xs_xi"]).max() < 1e-12
        assert np.abs(nu - o["us"]).max() < 1e-12


def test_r_to_q_restates_scipy_from_matrix():
    from scipy.spatial.transform import Rotation as Rot
    from tests.support import ORIENTATIONS
    rng = np.random.default_rng(2)
    Rs = [ob.se3_exp(np.r_[a * np.deg2rad(d), 0, 0, 0])[:3, :3] for a, d in ORIENTATIONS]
    Rs += [Rot.from_rotvec(v).as_matrix() for v in rng.normal(size=(64, 3)) * 2.0]
    seen = set()
    for R in Rs:
        q, br = r_to_q(R)
        seen.add(br)
        assert np.abs(q - Rot.from_matrix(R).as_quat()).max() < 1e-15
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("model", MODELS)
def test_case_grid_reaches_every_bucket(model):
    """The coverage guard of the eval_knot parity, on the knots it uses, and the reference's orientations through all four
    conversion branches, two of them with w < 0."""
    prob = large_rotation_problem(model_case(model, 1, N=22)[0])
    for i in (5, prob.N):
        ks = knot_states(prob, i)
        count = assert_coverage(ks["tags"])
        assert len(ks["tags"]) == 1024 and min(count.values()) >= 64
    conv = [r_to_q(prob.q_ref[i]) for i in range(prob.N + 1)]
    assert {br for _, br in conv} == {0, 1, 2, 3} and sum(q[3] < 0 for q, _ in conv) >= 4
