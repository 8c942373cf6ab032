"""Closed-loop covariance of the held policy (tolg_policy_covariance) against the CPU restatement of the recursion
(tests/restate.py: restate_covariance, from the oracle's fx_fu), fed the device's own gains and nominal:

- parity on every model, both shooting modes, at short horizons and ragged batches, with references and weights per trajectory;
- the exact properties: zeros, bitwise symmetry, var_x the diagonal's bits, PSD, independence of the batch, of repetition and of
  which outputs are asked for;
- the held policy is left alone, the handle's state rules, what the call ignores (plant, box, spheres), the full size.

The parity bound is the project's bound for costs, 1e-9, relative to the largest |Sigma| entry of the trajectory."""
import ctypes as C

import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, workloads
from tests.restate import restate_covariance
from tests.support import KW, MODELS, held_policy, host, model_case, moment_inputs, op_of, psd, same

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _check_parity(s, r, ops, S0r, Wr, c, what=""):
    """Every output of c (policy_covariance(full=True)) against the restatement, relative to max |Sigma| of the trajectory;
    returns the largest figure."""
    K = host(s.gains()["K"])
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    worst = 0.0
    for b in range(xq.shape[0]):
        Sig, var_x, var_u, pos = restate_covariance(ops[b], xq[b], xx[b], uu[b], K[b], S0r[b], Wr[b])
        scale = np.abs(Sig).max()
        errs = dict(Sigma=np.abs(host(c.Sigma)[b] - Sig).max() / scale, var_x=np.abs(host(c.var_x)[b] - var_x).max() / scale)
        errs["var_u"] = np.abs(host(c.var_u)[b] - var_u).max() / scale
        if c.pos_cov is not None:
            errs["pos_cov"] = np.abs(host(c.pos_cov)[b] - pos).max() / scale
        for k, e in errs.items():
            assert e < TOL, (what, b, k, e)
        worst = max(worst, *errs.values())
    print("%s parity %.2e" % (what, worst))
    return worst


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ms", "ss"])
@pytest.mark.parametrize("model", MODELS)
def test_parity_with_the_restatement(model, mode):
    B = 5
    prob, q, xi, us = model_case(model, B)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, mode)
    S0, W, S0r, Wr = moment_inputs(prob, B)
    c = s.policy_covariance(S0, W, full=True)
    assert (c.pos_cov is None) == (prob.kind in ("so3", "pendulum3d"))
    _check_parity(s, r, [op_of(prob)] * B, S0r, Wr, c, "%s %s" % (model, mode))


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("model", ["se3", "drone"])
def test_short_horizons_and_ragged_batches(model, N):
    """The terminal knot, a partly filled lane group (B = 1, 5: one trajectory in a block of four) and a partly filled
    wave; 67 = 16 blocks and three quarters."""
    for B in (1, 5, 17, 67):
        prob, q, xi, us = model_case(model, B, N=N)
        s = BatchedTrackingILQR(prob, B)
        r = held_policy(s, q, xi, us, "ms")
        S0, W, S0r, Wr = moment_inputs(prob, B, seed=B)
        c = s.policy_covariance(S0, W, full=True)
        _check_parity(s, r, [op_of(prob)] * B, S0r, Wr, c, "%s N=%d B=%d" % (model, N, B))
        assert same(c.Sigma, c.Sigma.transpose(2, 3))


# 3 -------------------------------------------------------------------------------------------------------------------
def test_parity_with_references_and_weights_per_trajectory():
    B = 3
    prob, q, xi, us, q_ref, xi_ref, idx, G = workloads.se3_multiref(B, 3, N=40)
    _, _, _, _, Q, P, R, _, _ = workloads.se3_weight_sweep(B, 3, N=40)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms", q_ref=q_ref, xi_ref=xi_ref, Q=Q, P=P, R=R)
    S0, W, S0r, Wr = moment_inputs(prob, B, seed=3)
    c = s.policy_covariance(S0, W, full=True)
    _check_parity(s, r, [op_of(prob, q_ref[b], xi_ref[b], Q[b], R[b], P[b]) for b in range(B)], S0r, Wr, c, "per-trajectory")


# 4 -------------------------------------------------------------------------------------------------------------------
def test_exact_properties():
    B, N = 5, 40
    prob, q, xi, us = workloads.se3_tracking(17, N=N)
    s = BatchedTrackingILQR(prob, B)
    held_policy(s, q[:B], xi[:B], us[:B], "ms")
    S0, W = psd(17, 12, 0.05, 1), psd(17, 6, 0.01, 2)
    z = s.policy_covariance(None, None, full=True)
    for t in (z.Sigma, z.var_x, z.var_u, z.pos_cov):
        assert not host(t).any()
    z = s.policy_covariance(np.zeros((12, 12)), np.zeros((B, 6, 6)), full=True)
    for t in (z.Sigma, z.var_x, z.var_u, z.pos_cov):
        assert not host(t).any()
    c = s.policy_covariance(S0[:B], W[:B], full=True)
    Sig = host(c.Sigma)
    assert np.isfinite(Sig).all()
    assert np.array_equal(Sig, np.swapaxes(Sig, 2, 3))
    assert np.array_equal(host(c.var_x), np.einsum("biaa->bia", Sig))
    assert same(c.pos_cov, c.pos_cov.transpose(2, 3))
    ev = np.linalg.eigvalsh(Sig)
    assert (ev[..., 0] >= -1e-12 * ev[..., -1]).all() and (host(c.var_u) >= 0).all()
    # only the upper triangles of the inputs are read
    S0l, Wl = S0[:B].copy(), W[:B].copy()
    S0l[:, np.tril_indices(12, -1)[0], np.tril_indices(12, -1)[1]] = 7.0
    Wl[:, np.tril_indices(6, -1)[0], np.tril_indices(6, -1)[1]] = -3.0
    f64 = dict(dtype=torch.float64, device=s.device)
    raw = torch.empty(B, N + 1, 12, 12, **f64)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    a, w = torch.as_tensor(S0l, **f64), torch.as_tensor(Wl, **f64)
    assert s.lib.tolg_policy_covariance(s._h, B, p(a), p(w), p(raw), None, None, None, s._stream()) == 0
    assert same(raw, c.Sigma)
    # two calls, and the reduced-only call: the same bits
    c2 = s.policy_covariance(S0[:B], W[:B], full=True)
    c3 = s.policy_covariance(S0[:B], W[:B])
    assert c3.Sigma is None
    for f in ("var_x", "var_u", "pos_cov"):
        assert same(getattr(c, f), getattr(c2, f)) and same(getattr(c, f), getattr(c3, f)), f
    assert same(c.Sigma, c2.Sigma)
    c4 = s.policy_covariance(S0[:B], W[:B], pos=False)
    assert c4.pos_cov is None and same(c4.var_x, c.var_x) and same(c4.var_u, c.var_u)
    # trajectory 2 of a batch of 5 in a batch of 17
    s17 = BatchedTrackingILQR(prob, 17)
    held_policy(s17, q, xi, us, "ms")
    c17 = s17.policy_covariance(S0, W, full=True)
    for f in ("Sigma", "var_x", "var_u", "pos_cov"):
        assert same(getattr(c, f)[2], getattr(c17, f)[2]), f


# 5 -------------------------------------------------------------------------------------------------------------------
def test_the_policy_is_left_alone_and_constraints_and_plants_are_ignored():
    B, N = 4, 40
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    s.fit_batch(q, xi, us, mode="ms", **KW)  # the policy a solve leaves, as it is
    S0, W = psd(B, 12, 0.05, 4), psd(B, 6, 0.01, 5)
    rng = np.random.default_rng(6)
    dx0, w = rng.normal(0, 0.03, (B, 3, 12)), rng.normal(0, 0.01, (B, 3, N, 6))
    g0, p0 = s.gains(), s.policy_rollout(dx0, w, trajectories=True)
    c0 = s.policy_covariance(S0, W, full=True)
    g1, p1 = s.gains(), s.policy_rollout(dx0, w, trajectories=True)
    assert same(g0["K"], g1["K"]) and same(g0["k"], g1["k"])
    for f in ("J", "status", "xs_q", "xs_xi", "us"):
        assert same(getattr(p0, f), getattr(p1, f)), f

    def same_as_c0():
        c = s.policy_covariance(S0, W, full=True)
        return all(same(getattr(c, f), getattr(c0, f)) for f in ("Sigma", "var_x", "var_u", "pos_cov"))

    f64 = dict(dtype=torch.float64, device=s.device)
    J = np.broadcast_to(np.asarray(prob.J, float) * 1.3, (B, 6, 6))
    s._set_plant(B, s._check_plant(B, J, None, per_sample=True))
    try:
        assert same_as_c0()
    finally:
        s._clear_plant()
    s.set_al(-0.1 * np.ones(prob.m), 0.1 * np.ones(prob.m), torch.ones(B, N, 2 * prob.m, **f64), torch.ones(B, N, 2 * prob.m, **f64))
    try:
        assert same_as_c0()
    finally:
        s.set_al(None)
    s.set_al_obstacles(np.array([[0.5, 0.0, 0.0, 0.3]]), torch.ones(B, N + 1, 1, **f64), torch.ones(B, N + 1, 1, **f64))
    try:
        assert same_as_c0()
    finally:
        s.set_al_obstacles(None)
    assert same_as_c0()


# 6 -------------------------------------------------------------------------------------------------------------------
def _raw(s, B, pos=False):
    f64 = dict(dtype=torch.float64, device=s.device)
    vx = torch.empty(B, s.N + 1, 12, **f64)
    pc = torch.empty(B, s.N + 1, 6, **f64) if pos else None
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    rc = s.lib.tolg_policy_covariance(s._h, B, None, None, None, p(vx), None, p(pc), s._stream())
    torch.cuda.synchronize()
    return rc


def test_handle_state_rules():
    B = 4
    prob, q, xi, us = workloads.se3_tracking(B, N=20)
    s = BatchedTrackingILQR(prob, B)
    assert _raw(s, B) == -1
    with pytest.raises(ValueError):
        s.policy_covariance()
    s.solve_begin(q, xi, us, mode="ms", **KW)
    assert _raw(s, B) == -1
    with pytest.raises(ValueError):
        s.policy_covariance()
    s.solve_iterate(4)
    s.solve_end()
    assert _raw(s, B) == 0 and _raw(s, B, pos=True) == 0
    assert _raw(s, B - 1) == -1
    # the host checks come before the device
    bad = np.eye(12); bad[0, 1] = 0.5
    for kw in (dict(Sigma0=bad), dict(W=-np.eye(6)), dict(Sigma0=np.full((12, 12), np.nan)), dict(W=np.eye(5)),
               dict(Sigma0=np.zeros((B + 1, 12, 12))), dict(Sigma0=np.eye(6))):
        with pytest.raises(ValueError):
            s.policy_covariance(**kw)
    # references per trajectory set for another batch
    prob3, q3, xi3, us3, q_ref, xi_ref, _, _ = workloads.se3_multiref(3, 3, N=20)
    s3 = BatchedTrackingILQR(prob3, B)
    s3.fit_batch(q3, xi3, us3, mode="ms", q_ref=q_ref, xi_ref=xi_ref, **KW)
    assert _raw(s3, 3) == 0 and _raw(s3, B) == -1


def test_pos_cov_is_refused_without_a_translation():
    for model in ("so3", "pendulum"):
        prob, q, xi, us = model_case(model, 3)
        s = BatchedTrackingILQR(prob, 3)
        s.fit_batch(q, xi, us, mode="ms", **KW)
        assert _raw(s, 3) == 0 and _raw(s, 3, pos=True) == -1
        assert s.policy_covariance(np.eye(6) * 1e-4, np.eye(3) * 1e-6).pos_cov is None


# 7 -------------------------------------------------------------------------------------------------------------------
def test_full_size():
    B, N = 4096, 200
    prob, q, xi, us, S0, W = workloads.se3_covariance(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    s.fit_batch(q, xi, us, mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
    c = s.policy_covariance(S0, W)
    assert c.Sigma is None
    for t in (c.var_x, c.var_u, c.pos_cov):
        assert np.isfinite(host(t)).all()
    assert (host(c.var_x) >= 0).all() and (host(c.var_u) >= 0).all()
    pc = host(c.pos_cov)[:, ::25]
    ev = np.linalg.eigvalsh(pc)
    assert (ev[..., 0] >= -1e-12 * ev[..., -1]).all()
