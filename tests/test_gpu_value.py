"""Cost-to-go of the held policy (tolg_policy_value) against the CPU restatement of the recursion (tests/restate.py,
from the oracle's fx_fu and cost), fed the device's own gains and nominal:

- parity on every model, both shooting modes, at short horizons and ragged batches, with references and weights per trajectory;
- the cross-kernel identity with tolg_policy_covariance on the device;
- the exact properties: bitwise symmetry, diag_P the diagonal's bits, zeros for zero inputs, independence of the batch, of
  repetition and of which outputs are asked for;
- the held policy is left alone, what the call ignores (plant, box, spheres), the handle's state rules, the full size.

The parity bound is the project's 1e-9: relative to max |P| of the trajectory for P, p and diag_P, to |excess| for price and
excess."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, workloads
from tests.restate import restate_stage_weights, restate_value
from tests.support import KW, MODELS, held_policy, host, model_case, moment_inputs, op_of, psd, same

pytestmark = pytest.mark.gpu
TOL = 1e-9
FIELDS = ("P", "p", "diag_P", "price", "excess")


def _check_parity(s, r, ops, S0r, Wr, v, what=""):
    """Every output of v (policy_value(full=True)) against the restatement; returns the largest figure."""
    K = host(s.gains()["K"])
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    worst = 0.0
    for b in range(xq.shape[0]):
        P, p, diag_P, price, excess = restate_value(ops[b], xq[b], xx[b], uu[b], K[b], S0r[b], Wr[b])
        scale = np.abs(P).max()
        errs = dict(P=np.abs(host(v.P)[b] - P).max() / scale, p=np.abs(host(v.p)[b] - p).max() / scale,
                    diag_P=np.abs(host(v.diag_P)[b] - diag_P).max() / scale,
                    price=np.abs(host(v.price)[b] - price).max() / abs(excess),
                    excess=abs(host(v.excess)[b] - excess) / abs(excess))
        for k, e in errs.items():
            assert e < TOL, (what, b, k, e)
        worst = max(worst, *errs.values())
    print("%s parity %.2e" % (what, worst))
    return worst


# 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ms", "ss"])
@pytest.mark.parametrize("model", MODELS)
def test_parity_with_the_restatement(model, mode):
    B = 5
    prob, q, xi, us = model_case(model, B)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, mode)
    S0, W, S0r, Wr = moment_inputs(prob, B)
    v = s.policy_value(S0, W, full=True)
    _check_parity(s, r, [op_of(prob)] * B, S0r, Wr, v, "%s %s" % (model, mode))


# 7 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("model", ["se3", "drone"])
def test_short_horizons_and_ragged_batches(model, N):
    """The terminal knot alone, a partly filled lane group (B = 1, 5: one trajectory in a block of four) and a partly filled
    wave; 67 = 16 blocks and three quarters."""
    for B in (1, 5, 17, 67):
        prob, q, xi, us = model_case(model, B, N=N)
        s = BatchedTrackingILQR(prob, B)
        r = held_policy(s, q, xi, us, "ms")
        S0, W, S0r, Wr = moment_inputs(prob, B, seed=B)
        v = s.policy_value(S0, W, full=True)
        _check_parity(s, r, [op_of(prob)] * B, S0r, Wr, v, "%s N=%d B=%d" % (model, N, B))
        assert same(v.P, v.P.transpose(2, 3))


# 8 -------------------------------------------------------------------------------------------------------------------
def test_parity_with_references_and_weights_per_trajectory():
    B = 3
    prob, q, xi, us, q_ref, xi_ref, idx, G = workloads.se3_multiref(B, 3, N=40)
    _, _, _, _, Q, P, R, _, _ = workloads.se3_weight_sweep(B, 3, N=40)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms", q_ref=q_ref, xi_ref=xi_ref, Q=Q, P=P, R=R)
    S0, W, S0r, Wr = moment_inputs(prob, B, seed=3)
    v = s.policy_value(S0, W, full=True)
    ops = [op_of(prob, q_ref[b], xi_ref[b], Q[b], R[b], P[b]) for b in range(B)]
    _check_parity(s, r, ops, S0r, Wr, v, "per-trajectory")
    # the trajectories differ: the kernel read each one's own reference and weights
    assert not same(v.P[0], v.P[1]) and not same(v.P[1], v.P[2])


# 9 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["se3", "drone"])
def test_cross_kernel_identity_with_the_covariance(model):
    """excess of tolg_policy_value equals sum_i tr(M_i Sigma_i) / 2 with Sigma_i from tolg_policy_covariance(full) on the
    device and M_i from the oracle's cost: two kernels, two directions, one number."""
    B = 5
    prob, q, xi, us = model_case(model, B, N=40)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms")
    S0, W, _, _ = moment_inputs(prob, B, seed=9)
    v = s.policy_value(S0, W)
    Sig = host(s.policy_covariance(S0, W, full=True).Sigma)
    K = host(s.gains()["K"])
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    for b in range(B):
        dual = 0.5 * np.einsum("iab,iba->", restate_stage_weights(op_of(prob), xq[b], xx[b], uu[b], K[b]), Sig[b])
        err = abs(host(v.excess)[b] - dual) / abs(dual)
        print("%s b=%d excess %.6g identity %.2e" % (model, b, dual, err))
        assert err < TOL, (b, err)


# 10 ------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    B, N = 5, 40
    prob, q, xi, us = workloads.se3_tracking(17, N=N)
    s = BatchedTrackingILQR(prob, B)
    held_policy(s, q[:B], xi[:B], us[:B], "ms")
    S0, W = psd(17, 12, 0.05, 1), psd(17, 6, 0.01, 2)
    v = s.policy_value(S0[:B], W[:B], full=True)
    Pm = host(v.P)
    assert np.isfinite(Pm).all() and np.isfinite(host(v.p)).all()
    assert np.array_equal(Pm, np.swapaxes(Pm, 2, 3))
    assert np.array_equal(host(v.diag_P), np.einsum("biaa->bia", Pm))
    assert (host(v.price) > 0).all() and (host(v.excess) > 0).all()
    # zero or absent inputs: exact zeros in price and excess, P and p unchanged
    for z in (s.policy_value(None, None, full=True), s.policy_value(np.zeros((12, 12)), np.zeros((B, 6, 6)), full=True),
              s.policy_value(None, np.zeros((6, 6)), full=True)):
        assert not host(z.price).any() and not host(z.excess).any()
        assert same(z.P, v.P) and same(z.p, v.p) and same(z.diag_P, v.diag_P)
    # only the upper triangles of the inputs are read
    S0l, Wl = S0[:B].copy(), W[:B].copy()
    S0l[:, np.tril_indices(12, -1)[0], np.tril_indices(12, -1)[1]] = 7.0
    Wl[:, np.tril_indices(6, -1)[0], np.tril_indices(6, -1)[1]] = -3.0
    f64 = dict(dtype=torch.float64, device=s.device)
    price, excess = torch.empty(B, N, **f64), torch.empty(B, **f64)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    a, w = torch.as_tensor(S0l, **f64), torch.as_tensor(Wl, **f64)
    assert s.lib.tolg_policy_value(s._h, B, p(a), p(w), None, None, None, p(price), p(excess), s._stream()) == 0
    assert same(price, v.price) and same(excess, v.excess)
    # two calls, and the reduced-only call: the same bits
    v2 = s.policy_value(S0[:B], W[:B], full=True)
    v3 = s.policy_value(S0[:B], W[:B])
    assert v3.P is None
    for f in FIELDS[1:]:
        assert same(getattr(v, f), getattr(v2, f)) and same(getattr(v, f), getattr(v3, f)), f
    assert same(v.P, v2.P)
    # a single output asked for: the same bits again (p is skipped when it is not)
    dg = torch.empty(B, N + 1, 12, **f64)
    assert s.lib.tolg_policy_value(s._h, B, None, None, None, None, p(dg), None, None, s._stream()) == 0
    assert same(dg, v.diag_P)
    # trajectory 2 of a batch of 5 in a batch of 17
    s17 = BatchedTrackingILQR(prob, 17)
    held_policy(s17, q, xi, us, "ms")
    v17 = s17.policy_value(S0, W, full=True)
    for f in FIELDS:
        assert same(getattr(v, f)[2], getattr(v17, f)[2]), f


# 11 ------------------------------------------------------------------------------------------------------------------
def test_the_policy_is_left_alone_and_constraints_and_plants_are_ignored():
    B, N = 4, 40
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    s.fit_batch(q, xi, us, mode="ms", **KW)  # the policy a solve leaves, as it is
    S0, W = psd(B, 12, 0.05, 4), psd(B, 6, 0.01, 5)
    rng = np.random.default_rng(6)
    dx0, w = rng.normal(0, 0.03, (B, 3, 12)), rng.normal(0, 0.01, (B, 3, N, 6))
    g0, p0 = s.gains(), s.policy_rollout(dx0, w, trajectories=True)
    v0 = s.policy_value(S0, W, full=True)
    g1, p1 = s.gains(), s.policy_rollout(dx0, w, trajectories=True)
    assert same(g0["K"], g1["K"]) and same(g0["k"], g1["k"])
    for f in ("J", "status", "xs_q", "xs_xi", "us"):
        assert same(getattr(p0, f), getattr(p1, f)), f

    def same_as_v0():
        v = s.policy_value(S0, W, full=True)
        return all(same(getattr(v, f), getattr(v0, f)) for f in FIELDS)

    f64 = dict(dtype=torch.float64, device=s.device)
    J = np.broadcast_to(np.asarray(prob.J, float) * 1.3, (B, 6, 6))
    s._set_plant(B, s._check_plant(B, J, None, per_sample=True))
    try:
        assert same_as_v0()
    finally:
        s._clear_plant()
    s.set_al(-0.1 * np.ones(prob.m), 0.1 * np.ones(prob.m), torch.ones(B, N, 2 * prob.m, **f64), torch.ones(B, N, 2 * prob.m, **f64))
    try:
        assert same_as_v0()
    finally:
        s.set_al(None)
    s.set_al_obstacles(np.array([[0.5, 0.0, 0.0, 0.3]]), torch.ones(B, N + 1, 1, **f64), torch.ones(B, N + 1, 1, **f64))
    try:
        assert same_as_v0()
    finally:
        s.set_al_obstacles(None)
    assert same_as_v0()


# 12 ------------------------------------------------------------------------------------------------------------------
def _raw(s, B):
    f64 = dict(dtype=torch.float64, device=s.device)
    dg = torch.empty(B, s.N + 1, 12, **f64)
    rc = s.lib.tolg_policy_value(s._h, B, None, None, None, None, C.c_void_p(dg.data_ptr()), None, None, s._stream())
    torch.cuda.synchronize()
    return rc


def test_handle_state_rules():
    B = 4
    prob, q, xi, us = workloads.se3_tracking(B, N=20)
    s = BatchedTrackingILQR(prob, B)
    assert _raw(s, B) == -1  # no policy
    with pytest.raises(ValueError):
        s.policy_value()
    s.solve_begin(q, xi, us, mode="ms", **KW)
    assert _raw(s, B) == -1  # a solve in flight
    with pytest.raises(ValueError):
        s.policy_value()
    s.solve_iterate(4)
    s.solve_end()
    assert _raw(s, B) == 0
    s.policy_value()
    assert _raw(s, B - 1) == -1  # another B
    s3m = BatchedTrackingILQR(prob, B)
    s3m.fit_batch(q[:3], xi[:3], us[:3], mode="ms", **KW)
    s3m._policy_B = B  # the method's own bookkeeping bypassed: the C call's refusal surfaces as ValueError
    with pytest.raises(ValueError):
        s3m.policy_value()
    s3m._policy_B = 3
    # the host checks come before the device
    bad = np.eye(12); bad[0, 1] = 0.5
    for kw in (dict(Sigma0=bad), dict(W=-np.eye(6)), dict(Sigma0=np.full((12, 12), np.nan)), dict(W=np.eye(5)),
               dict(Sigma0=np.zeros((B + 1, 12, 12))), dict(Sigma0=np.eye(6))):
        with pytest.raises(ValueError):
            s.policy_value(**kw)
    # references per trajectory set for another batch
    prob3, q3, xi3, us3, q_ref, xi_ref, _, _ = workloads.se3_multiref(3, 3, N=20)
    s3 = BatchedTrackingILQR(prob3, B)
    s3.fit_batch(q3, xi3, us3, mode="ms", q_ref=q_ref, xi_ref=xi_ref, **KW)
    assert _raw(s3, 3) == 0 and _raw(s3, B) == -1
    s3.policy_value()
    s3._policy_B = B
    with pytest.raises(ValueError):
        s3.policy_value()
    s3._policy_B = 3


# 13 ------------------------------------------------------------------------------------------------------------------
def test_full_size():
    B, N = 4096, 200
    prob, q, xi, us, S0, W = workloads.se3_covariance(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    s.fit_batch(q, xi, us, mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
    v = s.policy_value(S0, W)
    assert v.P is None
    for t in (v.p, v.diag_P, v.price, v.excess):
        assert np.isfinite(host(t)).all()
    assert (host(v.diag_P) >= 0).all() and (host(v.price) >= 0).all()
    # the position block of every 25th knot, on a slice of 64 trajectories with the full output
    s64 = BatchedTrackingILQR(prob, 64)
    s64.fit_batch(q[:64], xi[:64], us[:64], mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
    Pm = host(s64.policy_value(S0[:64], W[:64], full=True).P)[:, ::25, 3:6, 3:6]
    ev = np.linalg.eigvalsh(Pm)
    assert (ev[..., 0] >= -1e-12 * ev[..., -1]).all()
