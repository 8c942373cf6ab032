"""Large-rotation and per-trajectory parity of the newer policy kernels, which tests/test_gpu_large_rotation.py does not reach:
k_policy_rollout_est (its own Log and Exp sites, dyn_f, two chains in a quad), k_policy_rollout under a box (roll_step with the clamp
inside), pc_build_acl behind k_policy_covariance, k_policy_value and k_policy_covariance_est (closed-form so3_coef, so3_exp),
pv_cost of the value kernel, and the forms of the first two and of k_mpc_advance under a box with a reference and / or weights per
trajectory, in both sample orders.  The inputs and their guards are tests/support.py's (large_policy_case, large_estimated_case,
large_value_case), the guards themselves are asserted on the CPU restatements before the first launch, and
tests/test_large_rotation_policy_cpu.py asserts them again with the oracle's gains, where no device is needed.

  A. tolg_policy_rollout_estimated with start deviations, twist noise and measurement noise from the rotation grid and gains L
     of the test's own (filter_gains: the estimate jumps most of the way to a measurement radians off), every coordinate
     measured and the pose alone, against restate_rollout_estimated fed the device's gains K; both sample orders, bit for bit;
     one ragged case of 35 quads.
  B. tolg_policy_rollout_limited on the same perturbations, box from the unlimited restatement, against
     restate_policy_limited; both sample orders; an infinite box gives tolg_policy_rollout's bits.
  C. tolg_policy_covariance, tolg_policy_covariance_estimated and tolg_policy_value about nominals whose step rotations run
     over every Exp tier (beyond pi included) and whose tracking errors run over every Log tier, against restate_covariance,
     restate_covariance_estimated and restate_value.
  D. A, B and tolg_mpc_advance_limited with references per trajectory, weights per trajectory, and both, each with a control:
     the device's J is not the one the shared reference and weights give.

Bounds: the project's.  check_restatement's for the sampled loops (states 1e-10, inputs and u_excess 1e-8, J 1e-9 relative,
n_sat exact away from a bound), 1e-9 of the trajectory's max |Sigma| or max |P| for C (L absolute), check_advance's for the
advance (1e-13, J_cl 1e-12).  No bucket needed a bound of its own.

What the bounds rest on, all measured on the CPU on the inputs of these tests (tests/test_large_rotation_policy_cpu.py prints
and asserts every figure):
  - A, B: the spread of the restatement when K (and L) move by 1e-15 relative, per sample.  A sample is compared where eight
    times its spread is below the bounds in every field (tests/support.py::determined, the rule of the rollouts of
    tests/test_gpu_large_rotation.py); at least three quarters of a case's samples must be.  All are, except in A for the drone at
    N = 4 with the twist measured, 151 and 152 of 160: there 0.05 N(0, 1) of a twist innovation of 1e3 rad/s throws the
    estimate's position 1e2 from the path, where 1e-10 absolute is 1e-12 relative.  Worst spread over the compared samples,
    A: poses 1.3e-14 (the estimate's 5.1e-13, the drone's at N = 4 1.2e-11), twists 3.6e-12, inputs 7.3e-11 (drone, N = 4),
    J 4.6e-15; B: poses 7.8e-15, twists 1.4e-12, inputs 1.1e-11, u_excess 4.4e-11, J 3.1e-15.  With the oracle's gains every
    sample of A and B is finite, none of B lies near a bound, and 46 to 80 of 160 saturate (the drone at N = 4: box_widen).
  - C: the fp64 restatement against the same recursion in long double on oracle.bridge_ld.lin_backward's F_x, l_x, l_xx, the
    oracle's gains on both sides: at worst 3.1e-13 of max |Sigma| (so3, "tiers"), 2.0e-13 of max |P| for P and 9.2e-13 for p
    (se3, "tiers").  All 8 trajectories keep finite gains on the oracle.  The guard leaves out "wneg_small", which these
    trajectories do not hold (tests/support.py: VALUE_NEED).
The worst figures of a GPU run are printed by every test and kept in profiles/large_rotation_parity.txt."""
import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, workloads
from tests.checks import compare_estimated, compare_limited, limited_conditions, limited_guard
from tests.estimated import (estimated_guard, estimated_inputs, masks_of, restate_covariance_estimated, restate_estimated_batch)
from tests.limits import clamp, near_bound, restate_limited_batch
from tests.restate import restate_covariance, restate_value
from tests.support import (POLICY_B, VALUE_B, Nominal, box_widen, determined, filter_gains, host, large_estimated_case,
                           large_policy_case, large_value_case, moment_inputs, nudged, op_of, pert, policy_handle, rel,
                           same, sample_spread, value_guard)

pytestmark = pytest.mark.gpu

KINDS = ["se3", "drone", "so3"]
ROLLOUT = ("J", "status", "xs_q", "xs_xi", "us")
ESTIMATED = ROLLOUT + ("est_q", "est_xi")
LIMITED = ROLLOUT + ("n_sat", "u_excess")
TOL = 1e-9   # C: of max |Sigma| / max |P|


def _show(what, w):
    print(what, {k: "%.1e" % v for k, v in sorted(w.items())})


def _oracle_gains(op, nom):
    return np.array([ob.lin_backward(op, nom.xs_q[b], nom.xs_xi[b], nom.us[b], ms=True)["K"] for b in range(nom.us.shape[0])])


def _held(prob, nom, fast):
    """A handle in one of the two sample orders that holds the nominal through linearize_backward; (handle, its gains K)."""
    s = policy_handle(prob, nom.us.shape[0], fast)
    s.linearize_backward(nom.xs_q, nom.xs_xi, nom.us, ms=True)
    return s, host(s.gains()["K"])


def _keep(R, R2):
    return determined(sample_spread(R, R2))


# ---- A. tolg_policy_rollout_estimated --------------------------------------------------------------------------------------
def _estimated(kind, N, layout, pose_only, S, least):
    prob, nom, dx0, w, n, mask, L = large_estimated_case(kind, N, layout, pose_only, S)
    op = op_of(prob)
    B = POLICY_B
    estimated_guard(op, prob, nom, _oracle_gains(op, nom), L, mask, dx0, w, n, least=least)   # before any launch
    out = []
    for fast in (False, True):
        s, K = _held(prob, nom, fast)
        out.append((K, s.policy_rollout_estimated(L, mask, dx0, w, n, trajectories=True, estimates=True)))
    K, p = out[0]
    rng = np.random.default_rng(5)
    R = restate_estimated_batch([op] * B, nom, K, L, mask, dx0, w, n)
    keep = _keep(R, restate_estimated_batch([op] * B, nom, nudged(K, rng), nudged(L, rng), mask, dx0, w, n))
    assert 4 * int(keep.sum()) >= 3 * keep.size
    worst = compare_estimated(p, R, keep)
    _show("estimated %s N=%d S=%d %s %#05x (%d of %d compared)" % (kind, N, S, layout, mask, int(keep.sum()), keep.size), worst)
    for f in ESTIMATED:   # the other sample order: the same bits
        assert same(getattr(p, f), getattr(out[1][1], f)), f


@pytest.mark.parametrize("pose_only", [False, True], ids=["all", "pose"])
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_estimated_loop_with_large_innovations(kind, N, layout, pose_only):
    """Every tier of the innovation's and the estimate's Log, of the Exp of the measurement noise, of L_i r and of both chains'
    steps (tests/support.py::estimated_need), 16 samples of one trajectory per wave."""
    _estimated(kind, N, layout, pose_only, 32, least=4)


def test_estimated_loop_in_a_partly_filled_wave():
    """B S = 35 quads: the wave's last 13 replay the last sample and store nothing, in either sample order."""
    _estimated("se3", 4, "mixed", False, 7, least=0)


# ---- B. tolg_policy_rollout_limited ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_limited_loop_with_large_perturbations(kind, N, layout):
    prob, nom, dx0, w = large_policy_case(kind, N, layout)
    op = op_of(prob)
    B = POLICY_B
    lb, ub, _, _, _ = limited_guard(op, prob, nom, _oracle_gains(op, nom), dx0, w, box_widen(kind, N))   # before any launch
    out = []
    for fast in (False, True):
        s, K = _held(prob, nom, fast)
        out.append((K, s.policy_rollout(dx0, w, trajectories=True, u_lb=lb, u_ub=ub)))
    K, p = out[0]
    _, _, R = restate_limited_batch([op] * B, nom, K, dx0, w, box=(lb, ub))
    _, _, R2 = restate_limited_batch([op] * B, nom, nudged(K, np.random.default_rng(5)), dx0, w, box=(lb, ub))
    keep = _keep(R, R2)
    assert 4 * int(keep.sum()) >= 3 * keep.size
    fin, near = limited_conditions(R, lb, ub)
    worst = compare_limited(p, R, fin, near, keep)
    _show("limited %s N=%d %s (%d of %d compared)" % (kind, N, layout, int((fin & keep).sum()), keep.size), worst)
    for f in LIMITED:
        assert same(getattr(p, f), getattr(out[1][1], f)), f
    # an infinite box: the unlimited kernel's bits, on the same perturbations
    free = s.policy_rollout(dx0, w, trajectories=True)
    wide = s.policy_rollout(dx0, w, trajectories=True, u_lb=np.full(prob.m, -np.inf), u_ub=np.full(prob.m, np.inf))
    for f in ROLLOUT:
        assert same(getattr(free, f), getattr(wide, f)), f
    assert not host(wide.n_sat).any() and not host(wide.u_excess).any()


# ---- C. covariance, estimated covariance and value -------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [True, False], ids=["ms", "ss"])
@pytest.mark.parametrize("twists", ["sparse", "tiers"])
@pytest.mark.parametrize("kind", KINDS)
def test_covariance_and_value_about_large_rotation_nominals(kind, twists, ms):
    prob, xs_q, xs_xi, us, tags = large_value_case(kind, twists)
    value_guard(tags, twists)   # before any launch
    op = op_of(prob)
    B = VALUE_B
    s = BatchedTrackingILQR(prob, B)
    s.linearize_backward(xs_q, xs_xi, us, ms=ms)
    K = host(s.gains()["K"])
    kept = [b for b in range(B) if np.isfinite(K[b]).all()]   # "tiers" regularises some sweeps up to max_reg
    assert 4 * len(kept) >= 3 * B, kept
    S0, W, S0r, Wr = moment_inputs(prob, B)
    E0, EW, EV, E0r, EWr, EVr = estimated_inputs(prob, B)
    c = s.policy_covariance(S0, W, full=True)
    v = s.policy_value(S0, W, full=True)
    ce = {mask: s.policy_covariance_estimated(E0, EW, mask, EV, full=True, gains=True) for mask in masks_of(prob)}
    w = {}

    def within(name, e):
        w[name] = max(w.get(name, 0.0), float(e))
        assert e < TOL, (kind, twists, ms, b, name, float(e))

    for b in kept:
        a = (op, xs_q[b], xs_xi[b], us[b], K[b])
        Sig, var_x, var_u, pos = restate_covariance(*a, S0r[b], Wr[b])
        scale = np.abs(Sig).max()
        within("Sigma", np.abs(host(c.Sigma)[b] - Sig).max() / scale)
        within("var_x", np.abs(host(c.var_x)[b] - var_x).max() / scale)
        within("var_u", np.abs(host(c.var_u)[b] - var_u).max() / scale)
        if c.pos_cov is not None:
            within("pos_cov", np.abs(host(c.pos_cov)[b] - pos).max() / scale)
        P, p, diag_P, price, excess = restate_value(*a, S0r[b], Wr[b])
        scale = np.abs(P).max()
        within("P", np.abs(host(v.P)[b] - P).max() / scale)
        within("p", np.abs(host(v.p)[b] - p).max() / scale)
        within("diag_P", np.abs(host(v.diag_P)[b] - diag_P).max() / scale)
        within("price", np.abs(host(v.price)[b] - price).max() / abs(excess))
        within("excess", abs(host(v.excess)[b] - excess) / abs(excess))
        for mask, e in ce.items():
            o = restate_covariance_estimated(*a, mask, EVr[b], E0r[b], EWr[b])
            scale = np.abs(o["Sigma"]).max()
            for k in ("Sigma", "P_post", "L", "var_x", "var_est", "var_u", "pos_cov"):
                if k == "pos_cov" and e.pos_cov is None:
                    continue
                within("est:" + k, np.abs(host(getattr(e, k))[b] - o[k]).max() / (1.0 if k == "L" else scale))
    _show("covariance / value %s %s ms=%d (%d of %d trajectories)" % (kind, twists, ms, len(kept), B), w)


# ---- D. the forms with a reference or weights per trajectory ---------------------------------------------------------------
D_B, D_S, D_N, D_MASK = 3, 5, 40, 0x5A5


def _hold(hold):
    """(prob, q, xi, us, fit_batch's keywords, one OracleProblem per trajectory) of one hold on se3."""
    prob, q, xi, us, q_ref, xi_ref, _, _ = workloads.se3_multiref(D_B, 3, N=D_N)
    _, q_w, xi_w, _, Q, P, R, _, _ = workloads.se3_weight_sweep(D_B, 3, N=D_N)
    if hold == "references":
        return prob, q, xi, us, dict(q_ref=q_ref, xi_ref=xi_ref), [op_of(prob, q_ref[b], xi_ref[b]) for b in range(D_B)]
    if hold == "weights":   # (se3_tracking's starts: the references are not moved)
        return prob, q_w, xi_w, us, dict(Q=Q, P=P, R=R), [op_of(prob, Q=Q[b], R=R[b], P=P[b]) for b in range(D_B)]
    return (prob, q, xi, us, dict(q_ref=q_ref, xi_ref=xi_ref, Q=Q, P=P, R=R),
            [op_of(prob, q_ref[b], xi_ref[b], Q[b], R[b], P[b]) for b in range(D_B)])


def _control(what, J_dev, J_shared):
    """The sensitivity control: on the shared reference and weights the restatement's cost is another one."""
    off = np.abs(J_dev / J_shared - 1)
    print("%s: device J against the shared form's, relative: %s" % (what, np.array2string(off.max(axis=-1), precision=2)))
    assert (off > 1e-6).any(), what


@pytest.mark.parametrize("hold", ["references", "weights", "both"])
def test_per_trajectory_forms(hold):
    prob, q, xi, us, kw, ops = _hold(hold)
    shared = [op_of(prob)] * D_B
    dx0, w = pert(D_B, D_S, D_N, seed=12)
    n = np.random.default_rng(13).normal(size=(D_B, D_S, D_N + 1, 12)) * 0.02
    L = filter_gains(prob, D_B, D_MASK, seed=14)
    fit = dict(mode="ms", n_iterations=8, tol_grad_norm=0.0, tol_d_norm=0.0, **kw)
    out = []
    for fast in ((False, True) if hold == "both" else (False,)):
        s = policy_handle(prob, D_B, fast)
        r = s.fit_batch(q, xi, us, **fit)
        nom = Nominal(host(r.xs_q), host(r.xs_xi), host(r.us))
        K = host(s.gains()["K"])
        # the box, from the restatement with every trajectory's own reference and weights
        lb, ub, R = restate_limited_batch(ops, nom, K, dx0, w)
        out.append((s, nom, K, lb, ub, R, s.policy_rollout_estimated(L, D_MASK, dx0, w, n, trajectories=True, estimates=True),
                    s.policy_rollout(dx0, w, trajectories=True, u_lb=lb, u_ub=ub)))
    s, nom, K, lb, ub, R, pe, pl = out[0]
    # the estimated loop
    E = restate_estimated_batch(ops, nom, K, L, D_MASK, dx0, w, n)
    keep = np.ones((D_B, D_S), bool)
    assert sum(int(np.isfinite(e["J"]).sum()) for e in E) >= D_B * D_S // 2
    _show("per-trajectory %s, estimated" % hold, compare_estimated(pe, E, keep))
    _control("estimated, %s" % hold, host(pe.J), np.array([e["J"] for e in restate_estimated_batch(shared, nom, K, L, D_MASK, dx0, w, n)]))
    # the limited loop
    fin = np.array([np.isfinite(r_["J"]) for r_ in R])
    near = np.array([near_bound(r_["uc"], lb[b], ub[b]) for b, r_ in enumerate(R)])
    assert fin.sum() >= fin.size // 2 and sum(int(r_["n_sat"].sum()) for r_ in R) > 0
    _show("per-trajectory %s, limited" % hold, compare_limited(pl, R, fin, near))
    _control("limited, %s" % hold, host(pl.J), np.array([r_["J"] for r_ in restate_limited_batch(shared, nom, K, dx0, w, box=(lb, ub))[2]]))
    if hold == "both":   # the other sample order: the same bits
        for f in ESTIMATED:
            assert same(getattr(pe, f), getattr(out[1][6], f)), f
        for f in LIMITED:
            assert same(getattr(pl, f), getattr(out[1][7], f)), f
    # the advance with a box about u*_0 that cuts input 0 from below and input 3 from above (check_advance's bounds)
    u0 = nom.us[:, 0]
    alb, aub = u0 - 1.0, u0 + 1.0
    alb[:, 0], aub[:, 3] = u0[:, 0] + 0.1, u0[:, 3] - 0.1
    wa = np.random.default_rng(4).normal(0, 0.01, (D_B, 6))
    J1 = torch.zeros(D_B, dtype=torch.float64, device=s.device)
    a = s.mpc_advance(wa, J_cl=J1, u_lb=alb, u_ub=aub)
    want = clamp(u0, alb, aub)
    assert np.array_equal(host(a["u"]), want) and (host(a["n_sat"]) == 2).all()
    worst, J_own, J_shared = {}, np.zeros(D_B), np.zeros(D_B)
    for b in range(D_B):
        q1, x1 = ob.f(ops[b], nom.xs_q[b, 0], nom.xs_xi[b, 0], want[b])
        J_own[b] = ob.cost(ops[b], nom.xs_q[b, 0], nom.xs_xi[b, 0], want[b], 0)[0]
        J_shared[b] = ob.cost(shared[b], nom.xs_q[b, 0], nom.xs_xi[b, 0], want[b], 0)[0]
        for name, e, tol in (("x_next_q", rel(host(a["x_next_q"])[b], q1), 1e-13),
                             ("x_next_xi", rel(host(a["x_next_xi"])[b], x1 + wa[b]), 1e-13),
                             ("J_cl", abs(host(J1)[b] / J_own[b] - 1), 1e-12)):
            worst[name] = max(worst.get(name, 0.0), float(e))
            assert e < tol, (hold, b, name, float(e))
    _show("per-trajectory %s, advance" % hold, worst)
    _control("advance, %s" % hold, host(J1)[:, None], J_shared[:, None])
