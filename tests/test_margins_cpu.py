"""rollout_margins, the host definition of the margin report of the sampled closed loops (tolg_policy_rollout_margins,
tolg_policy_rollout_estimated_limited), and the keyword checks in front of those calls.  No GPU.

1. hand-built poses with known answers;  2. the first-knot rule on an exact tie;  3. NaN passed over, +inf when nothing is a
number;  4. counts and minima against a brute-force triple loop, numpy and torch alike;  5. on the oracle restatement's
trajectories: the counts sum over the sample axis, the minimum is the minimum of the per-knot minima, and the slot sets of the
device tests meet the conditions those tests assert;  6. the ValueError paths, on an instance without a handle."""
import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, rollout_margins, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import kind_clearance, pose_margin
from tests.estimated import held_policy_cpu
from tests.limits import restate_policy_limited
from tests.margins import (OBS_KINDS, POSE_KINDS, TILT, VIEW, brute_report, per_knot_minima, pose, pose_slots, position_slots,
                           rot)
from tests.support import model_case, pert

DEG = np.pi / 180.0


def _xs(poses):
    """[1, 1, n, 4, 4] from a list of poses: one trajectory, one sample."""
    return np.stack(poses)[None, None]


# 1 -------------------------------------------------------------------------------------------------------------------
def test_hand_built_poses():
    tilt = np.array([[0.0, 0.0, 1.0, np.cos(40 * DEG)]])
    r = rollout_margins(_xs([pose(rot([1, 0, 0], 30 * DEG))]), pose_slots=tilt, pose_kinds=[TILT])
    assert abs(r["pose_margin"][0, 0] - (np.cos(30 * DEG) - np.cos(40 * DEG))) < 1e-15
    assert r["pose_margin_knot"][0, 0] == 0 and r["viol_pose"].tolist() == [[0]]
    assert r["pose_margin_knot"].dtype == np.int32 and r["viol_pose"].dtype == np.int32
    # 30 degrees about any horizontal axis, and 50 degrees: outside by cos 50 - cos 40
    r = rollout_margins(_xs([pose(rot([0.6, 0.8, 0], 30 * DEG)), pose(rot([0, 1, 0], 50 * DEG))]), pose_slots=tilt, pose_kinds=["tilt_cone"])
    assert abs(r["pose_margin"][0, 0] - (np.cos(50 * DEG) - np.cos(40 * DEG))) < 1e-15
    assert r["pose_margin_knot"][0, 0] == 1 and r["viol_pose"].tolist() == [[0, 1]]
    # a view target dead ahead of a rotated, displaced pose: cosine 1; abeam (along e2): cosine 0
    R, t, c = rot([0.2, -0.5, 0.7], 1.1), np.array([0.3, -1.0, 2.0]), np.cos(25 * DEG)
    ahead, abeam = np.r_[t + 3.0 * R[:, 0], c], np.r_[t - 2.0 * R[:, 1], c]
    r = rollout_margins(_xs([pose(R, t)]), pose_slots=np.stack([ahead]), pose_kinds=[VIEW])
    assert abs(r["pose_margin"][0, 0] - (1.0 - c)) < 1e-15 and r["viol_pose"].tolist() == [[0]]
    r = rollout_margins(_xs([pose(R, t)]), pose_slots=np.stack([ahead, abeam]), pose_kinds=[VIEW, VIEW])
    assert abs(r["pose_margin"][0, 0] - (0.0 - c)) < 1e-15 and r["viol_pose"].tolist() == [[1]]
    # the position family: 0.25 inside a keep-out sphere at knot 1
    xs = _xs([pose(t=[2.0, 0, 0]), pose(t=[0.75, 0, 0]), pose(t=[0, 3.0, 0])])
    r = rollout_margins(xs, obstacles=np.array([[0.0, 0, 0, 1.0]]))
    assert r["clearance"][0, 0] == -0.25 and r["clearance_knot"][0, 0] == 1 and r["viol_pos"].tolist() == [[0, 1, 0]]
    assert "pose_margin" not in r and "viol_pose" not in r
    with pytest.raises(ValueError):
        rollout_margins(xs)
    with pytest.raises(ValueError):
        rollout_margins(xs[0], obstacles=np.array([[0.0, 0, 0, 1.0]]))
    with pytest.raises(ValueError):
        rollout_margins(xs, obstacles=np.zeros((2, 1, 4)))
    with pytest.raises(ValueError):
        rollout_margins(xs, pose_slots=tilt)  # pose slots have no default kind


# 2 -------------------------------------------------------------------------------------------------------------------
def test_first_knot_on_an_exact_tie():
    tilt = np.array([[0.0, 0.0, 1.0, 0.5]])
    tilted = pose(rot([1, 0, 0], 0.7))
    # knots 1 and 3 hold the very same pose: the very same margin, and the first of them is reported
    r = rollout_margins(_xs([pose(), tilted, pose(), tilted.copy(), pose()]), pose_slots=tilt, pose_kinds=[TILT])
    assert r["pose_margin_knot"][0, 0] == 1
    # the same within one knot across two slots does not move the knot; and in the position family
    r = rollout_margins(_xs([pose(), tilted, tilted.copy()]), pose_slots=np.concatenate([tilt, tilt]), pose_kinds=[TILT, TILT])
    assert r["pose_margin_knot"][0, 0] == 1
    xs = _xs([pose(t=[2.0, 0, 0]), pose(t=[0, 1.5, 0]), pose(t=[0, 0, -1.5]), pose(t=[0, -1.5, 0])])
    r = rollout_margins(xs, obstacles=np.array([[0.0, 0, 0, 1.0]]))
    assert r["clearance"][0, 0] == 0.5 and r["clearance_knot"][0, 0] == 1


# 3 -------------------------------------------------------------------------------------------------------------------
def test_nan_is_passed_over():
    view = np.array([[1.0, 2.0, 3.0, 0.5]])
    at_target, off = pose(t=[1.0, 2.0, 3.0]), pose(t=[0.0, 2.0, 3.0])  # b = 0: 0 / 0
    with np.errstate(invalid="ignore"):
        r = rollout_margins(_xs([at_target, off, at_target]), pose_slots=view, pose_kinds=[VIEW])
        assert r["pose_margin"][0, 0] == 0.5 and r["pose_margin_knot"][0, 0] == 1 and r["viol_pose"].tolist() == [[0, 0, 0]]
        r = rollout_margins(_xs([at_target, at_target]), pose_slots=view, pose_kinds=[VIEW])
        assert r["pose_margin"][0, 0] == np.inf and r["pose_margin_knot"][0, 0] == 0 and not r["viol_pose"].any()
        # a NaN pose at knot 0 with a violation behind it: knot 1 is counted and reported, knot 0 is not
        bad = pose()
        bad[:3, :3] = np.nan
        tilt = np.array([[0.0, 0.0, 1.0, 0.9]])
        r = rollout_margins(_xs([bad, pose(rot([1, 0, 0], 1.0))]), pose_slots=tilt, pose_kinds=[TILT])
        assert r["pose_margin"][0, 0] < 0 and r["pose_margin_knot"][0, 0] == 1 and r["viol_pose"].tolist() == [[0, 1]]
        xs = _xs([pose(t=[np.nan, 0, 0]), pose(t=[3.0, 0, 0])])
        r = rollout_margins(xs, obstacles=np.array([[0.0, 0, 0, 1.0]]))
        assert r["clearance"][0, 0] == 2.0 and r["clearance_knot"][0, 0] == 1 and not r["viol_pos"].any()


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["shared", "static", "per_knot"])
def test_against_a_brute_force_loop(form):
    B, S, N1 = 3, 4, 7
    rng = np.random.default_rng(3)
    xs = np.zeros((B, S, N1, 4, 4))
    for idx in np.ndindex(B, S, N1):
        xs[idx] = pose(rot(rng.normal(size=3), rng.uniform(0, 2.5)), rng.normal(size=3))
    pk, ok = POSE_KINDS[5], OBS_KINDS[5]
    shape = {"shared": (5, 4), "static": (B, 5, 4), "per_knot": (B, N1, 5, 4)}[form]
    ps = rng.normal(size=shape)
    ps[..., 0, :3] = [0.0, 0.0, 1.0]
    ps[..., 2, :3] = [0.6, 0.0, 0.8]
    ps[..., 3] = rng.uniform(-0.3, 0.6, size=shape[:-1])
    os_ = rng.normal(size=shape)
    os_[..., 1, :3] = [0.0, 0.6, 0.8]
    os_[..., 3] = rng.uniform(0.3, 1.5, size=shape[:-1])
    full = lambda a: np.broadcast_to(a if a.ndim == 4 else (a[:, None] if a.ndim == 3 else a[None, None]), (B, N1, 5, 4))  # noqa: E731
    mp = pose_margin(xs, full(ps)[:, None], pk)
    mc = kind_clearance(xs[..., :3, 3], full(os_)[:, None], ok)
    r = rollout_margins(xs, obstacles=os_, kinds=ok, pose_slots=ps, pose_kinds=pk)
    for m, names in ((mp, ("pose_margin", "pose_margin_knot", "viol_pose")), (mc, ("clearance", "clearance_knot", "viol_pos"))):
        best, knot, count = brute_report(m)
        assert np.array_equal(r[names[0]], best) and np.array_equal(r[names[1]], knot) and np.array_equal(r[names[2]], count)
        assert 0 < count.sum() < B * S * N1
    # torch gives the numbers numpy gives
    rt = rollout_margins(torch.as_tensor(xs), obstacles=os_, kinds=ok, pose_slots=torch.as_tensor(ps), pose_kinds=pk)
    for k, v in r.items():
        assert isinstance(rt[k], torch.Tensor) and rt[k].dtype == (torch.float64 if v.dtype == np.float64 else torch.int32)
        if v.dtype == np.float64:
            assert np.abs(rt[k].numpy() - v).max() < 1e-14, k
        elif not k.endswith("knot"):
            assert np.array_equal(rt[k].numpy(), v), k


# 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("per_knot", [False, True])
@pytest.mark.parametrize("model,B,S", [("se3", 3, 5), ("drone", 5, 7)])
def test_on_the_restated_closed_loops(model, B, S, per_knot, K):
    """The trajectories of tests/limits.py::restate_policy_limited about the oracle's policy, with the slot sets of the device
    tests: the conditions those tests assert on the device's trajectories hold on the restatement's."""
    N = 40
    prob, q, xi, us = model_case(model, B, N=N)
    dx0, w = pert(B, S, N, seed=11)
    nom, xs = [], []
    for b in range(B):
        op, xq, xx, uu, Kg = held_policy_cpu(prob, q[b], xi[b], us[b], "ms")
        nom.append(xq)
        xs.append(restate_policy_limited(op, xq, xx, uu, Kg, None, None, dx0[b], w[b], S)["xs_q"])
    nom, xs = np.stack(nom), np.stack(xs)
    ps, os_ = pose_slots(nom, POSE_KINDS[K], per_knot), position_slots(nom, OBS_KINDS[K], per_knot)
    r = rollout_margins(xs, obstacles=os_, kinds=OBS_KINDS[K], pose_slots=ps, pose_kinds=POSE_KINDS[K])
    for fam, viol, mins in (("pose_margin", "viol_pose", per_knot_minima(xs, pose=ps, pose_kinds=POSE_KINDS[K])),
                            ("clearance", "viol_pos", per_knot_minima(xs, obstacles=os_, kinds=OBS_KINDS[K]))):
        assert np.array_equal(r[viol], (mins < 0).sum(axis=1)) and r[viol].sum() == (mins < 0).sum()
        assert np.array_equal(r[fam], mins.min(axis=-1))
        assert np.array_equal(r[fam + "_knot"], mins.argmin(axis=-1))
        assert (r[fam] < 0).any() and (r[fam] > 0).any(), fam
        assert np.abs(mins).min() > 1e-9
        v = r[viol]
        print("%s K=%d per_knot=%d: counts 0: %d, S: %d, between: %d" % (viol, K, per_knot, (v == 0).sum(), (v == S).sum(),
                                                                         ((v > 0) & (v < S)).sum()))
        assert (v == 0).any() and (v == S).any() and ((v > 0) & (v < S)).any(), viol
    targets = ps[..., [k for k, kd in enumerate(POSE_KINDS[K]) if kd == VIEW], :3]
    if targets.size:
        tg = targets[:, None, None] if targets.ndim == 3 else targets[:, None]
        assert np.linalg.norm(xs[..., None, :3, 3] - tg, axis=-1).min() >= 0.5


# 6 -------------------------------------------------------------------------------------------------------------------
def test_keyword_checks_raise_value_error():
    """The checks of the new keywords come before anything reaches the device: exercised on an instance without a handle."""
    prob, *_ = workloads.se3_tracking(3, N=5)
    s = object.__new__(BatchedTrackingILQR)
    s.problem, s._policy_B, s._obs, s._pose, s.N, s.m = prob, 3, None, None, prob.N, prob.m
    L = np.zeros((3, 6, 12, 12))
    for call in (lambda **kw: s.policy_rollout(S=2, **kw), lambda **kw: s.policy_rollout_estimated(L, 0x03F, S=2, **kw)):
        with pytest.raises(ValueError, match="set_al_pose_constraints"):
            call(pose_margin=True)
        with pytest.raises(ValueError, match="constraint family"):
            call(violations=True)
        with pytest.raises(ValueError, match="set_al_obstacles"):
            call(clearance=True)
        s._obs = (None, None, None)  # position slots attached, no pose slots: pose_margin is still refused
        with pytest.raises(ValueError, match="set_al_pose_constraints"):
            call(pose_margin=True, violations=True)
        s._obs = None
    with pytest.raises(ValueError, match="come together"):
        s.policy_rollout_estimated(L, 0x03F, S=2, u_lb=np.zeros(6))
    s._policy_B = 0
    with pytest.raises(ValueError, match="no policy is held"):
        s.policy_rollout(S=2, pose_margin=True)
