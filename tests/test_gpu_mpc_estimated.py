"""Output feedback inside the receding-horizon loop on the device: tolg_mpc_measure, tolg_mpc_advance_estimated and
mpc(meas_* / est_*) against the CPU restatements of tests/mpc_estimated.py, fed the device's own nominal:

- the two calls against their restatements on every model, at the smallest shapes and at ragged batches;
- the exact identities with tolg_mpc_advance_limited and with mpc();
- the chain measure / advance / measure against the horizon sweep of tolg_policy_covariance_estimated;
- the loop step by step, with warm states, under a keep-out sphere and an actuator box; the filter's statistics;
- the argument rules, raw through the C ABI.

Bounds, the project's own for the same operations: tests/checks.py::check_advance's 1e-13 for a dynamics step and 1e-12 for a
stage cost; tests/test_gpu_estimated.py's 1e-9 of max |P| for covariances, 1e-9 absolute for L, 1e-10 for an estimate
correction (and the residual it is made from); check_loop's 1e-9 for J_hist and 1e-6 relative for us."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import mpc_shift
from tests.estimated import MASKS_EDGE, estimated_inputs, masks_of
from tests.mpc_estimated import (filter_case, filter_figures, restate_advance_estimated, restate_measure, upper)
from tests.restate import plant_problem, restate_mpc_step, window_problem
from tests.support import KW, MODELS, ZERO, dense_fixed_block, held_policy, host, model_case, op_of, psd, rel, same

pytestmark = pytest.mark.gpu
UNUSED = [3, 4, 5, 9, 10, 11]
ADV = ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us", "n_sat")


def dev(s, a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=s.device).contiguous()


def so3(prob):
    return prob.kind in ("so3", "pendulum3d")


def scattered(prob, q, xi, seed, pose, twist):
    """x (+) d with d ~ N(0, diag(pose, twist)^2), zero in the coordinates the SO3 family does not carry; d too."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(q.shape[0], 12)) * np.r_[[pose] * 6, [twist] * 6]
    if so3(prob):
        d[:, UNUSED] = 0.0
    return np.stack([np.asarray(q[b], float).reshape(4, 4) @ ob.se3_exp(d[b, :6]) for b in range(q.shape[0])]), xi + d[:, 6:], d


def check_measure(s, prob, q, xi, mask, seed=1, what=""):
    """tolg_mpc_measure on B states near (q, xi) against restate_measure: est, P, L, innov, var_est; P symmetric to the bit."""
    B = q.shape[0]
    S0, _, V, S0r, _, Vr = estimated_inputs(prob, B, seed=seed)
    xq, xx, _ = scattered(prob, q, xi, seed + 1, 0.05, 0.05)
    eq, ex, _ = scattered(prob, xq, xx, seed + 2, 0.01, 0.01)
    _, _, n = scattered(prob, xq, xx, seed + 3, 0.005, 0.005)
    P = np.triu(S0r) + 7.0 * np.tril(S0r, -1)  # the lower triangle is not read
    d_eq, d_ex, d_P = dev(s, eq), dev(s, ex), dev(s, P)
    o = s.mpc_measure(mask, V if mask else None, dev(s, xq), dev(s, xx), d_eq, d_ex, d_P, noise=n)
    gP = host(d_P)
    assert np.array_equal(gP, np.swapaxes(gP, 1, 2)), what
    assert np.array_equal(host(o["var_est"]), np.einsum("bii->bi", gP)), what
    worst = 0.0
    for b in range(B):
        r = restate_measure(xq[b], xx[b], eq[b], ex[b], P[b], mask, Vr[b], n[b])
        scale = np.abs(S0r[b]).max()
        figs = dict(est_q=np.abs(host(d_eq)[b] - r["est_q"]).max() / 1e-10, est_xi=np.abs(host(d_ex)[b] - r["est_xi"]).max() / 1e-10,
                    innov=np.abs(host(o["innov"])[b] - r["innov"]).max() / 1e-10, P=np.abs(gP[b] - r["P"]).max() / scale / 1e-9,
                    L=np.abs(host(o["L"])[b] - r["L"]).max() / 1e-9)
        for k, v in figs.items():
            assert v < 1.0, (what, b, k, v)
            worst = max(worst, v)
    print("%s mask %#05x measure: worst figure / bound %.2e" % (what, mask, worst))


def box_of(u0, seed):
    """A box about the first inputs u*_0 [B, m] that moves some of them: input 0 of every trajectory from above, a quarter of
    the others from either side."""
    rng = np.random.default_rng(seed)
    sd = np.abs(u0).max() + 1e-3
    lb = u0 - np.abs(rng.normal(size=u0.shape)) * sd + 0.5 * sd * (rng.uniform(size=u0.shape) < 0.25)
    ub = u0 + np.abs(rng.normal(size=u0.shape)) * sd - 0.5 * sd * (rng.uniform(size=u0.shape) < 0.25)
    lb, ub = np.minimum(lb, ub), np.maximum(lb, ub)
    ub[:, 0] = u0[:, 0] - 0.25 * sd
    lb[:, 0] = u0[:, 0] - sd
    return lb, ub


def check_advance_estimated(s, prob, r, seed=2, plant_J=None, what=""):
    """tolg_mpc_advance_estimated on the held policy r against restate_advance_estimated: x_true', x_next, the warm tail, J_cl, P',
    the applied input and the shift."""
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    B, N = uu.shape[:2]
    _, W, _, S0r, Wr, _ = estimated_inputs(prob, B, seed=seed)
    tq, tx, _ = scattered(prob, xq[:, 0], xx[:, 0], seed + 1, 0.01, 0.01)
    rng = np.random.default_rng(seed + 2)
    w = rng.normal(size=(B, 6)) * 0.01
    if so3(prob):
        w[:, 3:] = 0.0
    lb, ub = box_of(uu[:, 0], seed + 3)
    if so3(prob):
        lb[:, 3:], ub[:, 3:] = -np.inf, np.inf
    d_tq, d_tx, d_P = dev(s, tq), dev(s, tx), dev(s, S0r)
    J = torch.zeros(B, dtype=torch.float64, device=s.device)
    a = s.mpc_advance_estimated(d_tq, d_tx, d_P, w=w, W=W, J_cl=J, u_lb=lb, u_ub=ub, plant_J=plant_J)
    gP = host(d_P)
    assert np.array_equal(gP, np.swapaxes(gP, 1, 2)), what
    op = op_of(prob)
    moved = 0
    for b in range(B):
        o = restate_advance_estimated(op, xq[b], xx[b], uu[b], tq[b], tx[b], S0r[b], w[b], Wr[b], lb[b], ub[b],
                                      None if plant_J is None else plant_problem(prob, plant_J[b]))
        assert np.array_equal(host(a["u"])[b], o["u"]) and int(host(a["n_sat"])[b]) == o["n_sat"], (what, b)
        moved += o["n_sat"]
        assert rel(host(d_tq)[b], o["x_true_q"]) < 1e-13 and rel(host(d_tx)[b], o["x_true_xi"]) < 1e-13, (what, b)
        assert rel(host(a["x_next_q"])[b], o["x_next_q"]) < 1e-13 and rel(host(a["x_next_xi"])[b], o["x_next_xi"]) < 1e-13, (what, b)
        assert rel(host(a["xs_q"])[b, N], o["tail_q"]) < 1e-13 and rel(host(a["xs_xi"])[b, N], o["tail_xi"]) < 1e-13, (what, b)
        assert abs(host(J)[b] / o["dJ"] - 1) < 1e-12, (what, b)
        e = np.abs(gP[b] - o["P"]).max() / max(np.abs(o["P"]).max(), np.abs(S0r[b]).max())
        assert e < 1e-9, (what, b, e)
    assert moved > 0, what  # the box is on
    # the warm start: the bits of tolg_mpc_advance_limited's (the shift of the held solution, the model's two ends)
    lim = s.mpc_advance(u_lb=lb, u_ub=ub)
    assert same(a["xs_q"], lim["xs_q"]) and same(a["xs_xi"], lim["xs_xi"]) and same(a["us"], lim["us"]), what
    assert same(a["us"][:, :-1], uu[:, 1:]) and same(a["us"][:, -1], uu[:, -1]), what
    return a


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_measure_against_the_restatement(model):
    B = 5
    prob, q, xi, us = model_case(model, B)
    s = BatchedTrackingILQR(prob, B)
    for mask in masks_of(prob) + (MASKS_EDGE if model == "se3" else ()):
        check_measure(s, prob, np.asarray(q).reshape(B, 4, 4), xi, mask, what=model)


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_advance_against_the_restatement(model):
    B = 5
    prob, q, xi, us = model_case(model, B, N=40)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms")
    check_advance_estimated(s, prob, r, what=model)


@pytest.mark.parametrize("form", ["diagonal", "dense"])
def test_advance_on_a_plant_against_the_restatement(form):
    B = 5
    prob, q, xi, us = model_case("se3", B, N=40)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms")
    rng = np.random.default_rng(4)
    PJ = np.stack([np.diag(np.diag(prob.J) * np.exp(rng.normal(0, 0.1, 6))) for _ in range(B)])
    if form == "dense":
        PJ[:, :3, :3] = dense_fixed_block(prob).J[:3, :3] * np.exp(rng.normal(0, 0.1, (B, 1, 1)))
    a = check_advance_estimated(s, prob, r, plant_J=PJ, what=form)
    # the estimate's prior stays the model's: the bits of the call without a plant
    b = s.mpc_advance_estimated(dev(s, host(r.xs_q)[:, 0]), dev(s, host(r.xs_xi)[:, 0]), dev(s, np.zeros((B, 12, 12))))
    assert same(a["xs_q"][:, -1], b["xs_q"][:, -1]) and same(a["us"], b["us"])


# 3 -------------------------------------------------------------------------------------------------------------------
def test_exact_identities():
    B, N = 5, 40
    prob, q, xi, us = model_case("se3", B, N=N)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms")
    g0 = s.gains()
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    lb, ub = box_of(uu[:, 0], 5)
    rng = np.random.default_rng(6)
    w = rng.normal(size=(B, 6)) * 0.01
    PJ = np.stack([np.diag(np.diag(prob.J) * np.exp(rng.normal(0, 0.1, 6))) for _ in range(B)])
    tq, tx, _ = scattered(prob, xq[:, 0], xx[:, 0], 7, 0.05, 0.05)
    S0, W = psd(B, 12, 0.01, 8), psd(B, 6, 0.01, 9)
    lim = s.mpc_advance(u_lb=lb, u_ub=ub)
    assert int(host(lim["n_sat"]).sum()) > 0
    zero = torch.zeros(B, dtype=torch.float64, device=s.device)
    for plant in (None, PJ):
        # ends 0 and 1: tolg_mpc_advance_limited without a plant and without w, whatever the true state and the plant
        d_tq, d_tx, d_P = dev(s, tq), dev(s, tx), dev(s, S0)
        e = s.mpc_advance_estimated(d_tq, d_tx, d_P, w=w, W=W, u_lb=lb, u_ub=ub, plant_J=plant)
        for k in ADV:
            assert same(e[k], lim[k]), (k, plant is not None)
        # a second call with restored buffers: the same bits
        d_tq2, d_tx2, d_P2 = dev(s, tq), dev(s, tx), dev(s, S0)
        e2 = s.mpc_advance_estimated(d_tq2, d_tx2, d_P2, w=w, W=W, u_lb=lb, u_ub=ub, plant_J=plant)
        assert same(d_tq, d_tq2) and same(d_tx, d_tx2) and same(d_P, d_P2) and all(same(e[k], e2[k]) for k in ADV)
        # the third end with x_true = x*_0 to the bit: end 0 of tolg_mpc_advance_limited with w and the plant
        J1, J2 = zero.clone(), zero.clone()
        c = s.mpc_advance(w, J_cl=J1, u_lb=lb, u_ub=ub, plant_J=plant)
        d_tq, d_tx = dev(s, xq[:, 0]), dev(s, xx[:, 0])
        s.mpc_advance_estimated(d_tq, d_tx, dev(s, S0), w=w, J_cl=J2, u_lb=lb, u_ub=ub, plant_J=plant)
        assert same(d_tq.reshape(B, 4, 4), c["x_next_q"]) and same(d_tx, c["x_next_xi"]) and same(J1, J2), plant is not None
        assert host(J1).all()
    # without a box: tolg_mpc_advance's bits, n_sat = 0
    free, e = s.mpc_advance(), s.mpc_advance_estimated(dev(s, tq), dev(s, tx), dev(s, S0))
    assert all(same(e[k], free[k]) for k in ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us")) and not host(e["n_sat"]).any()
    # P = 0 with W None stays exact zeros
    d_P = dev(s, np.zeros((B, 12, 12)))
    s.mpc_advance_estimated(dev(s, tq), dev(s, tx), d_P)
    assert not host(d_P).any()
    # no sensor: the estimate's bits are left alone, L = 0, P is its mirrored upper triangle
    P = np.triu(S0) + 3.0 * np.tril(S0, -1)
    d_eq, d_ex, d_P = dev(s, tq), dev(s, tx), dev(s, P)
    o = s.mpc_measure(0, None, dev(s, xq[:, 0]), dev(s, xx[:, 0]), d_eq, d_ex, d_P, noise=w.repeat(2, axis=1))
    assert same(d_eq, tq) and same(d_ex, tx) and not host(o["L"]).any() and not host(o["innov"]).any()
    assert same(d_P, np.stack([upper(p) for p in P])) and same(o["var_est"], np.einsum("bii->bi", S0))
    # the held policy is left alone
    g1 = s.gains()
    assert same(g0["k"], g1["k"]) and same(g0["K"], g1["K"])


def test_the_loop_without_a_sensor_is_the_loop():
    B, steps, N = 4, 3, 20
    prob, q, xi, pq, px, t0, _ = workloads.se3_mpc(B, steps, N=N, seed=5)
    kw = dict(t0=t0, first_iters=4, iters_per_step=2, **ZERO)
    for warm in ("states", "controls"):
        a = BatchedTrackingILQR(prob, B).mpc(q, xi, pq, px, steps, warm=warm, **kw)
        e = BatchedTrackingILQR(prob, B).mpc(q, xi, pq, px, steps, warm=warm, meas_mask=0, **kw)
        for k in ("xs_q", "xs_xi", "us", "J"):
            assert same(getattr(a, k), getattr(e, k)), (warm, k)
        assert a.est_q is None and same(e.est_q, e.xs_q) and same(e.est_xi, e.xs_xi) and not host(e.est_var).any()


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["se3", "drone", "so3"])
def test_the_chain_is_the_horizon_sweep(model):
    """Device against device: measure(Sigma0), advance_estimated, measure on the held policy give P_post[:, 0], L[:, 0],
    P_post[:, 1], L[:, 1] of policy_covariance_estimated, to 1e-9 of scale (L absolutely)."""
    B = 5
    prob, q, xi, us = model_case(model, B, N=40)
    s = BatchedTrackingILQR(prob, B)
    r = held_policy(s, q, xi, us, "ms")
    S0, W, V, S0r, _, _ = estimated_inputs(prob, B)
    for mask in masks_of(prob):
        c = s.policy_covariance_estimated(S0, W, mask, V, full=True, gains=True)
        scale = np.abs(host(c.Sigma)).reshape(B, -1).max(axis=1)[:, None, None]
        x0q, x0x = dev(s, host(r.xs_q)[:, 0]), dev(s, host(r.xs_xi)[:, 0])
        d_eq, d_ex, d_P = x0q.clone(), x0x.clone(), dev(s, S0r)
        for i in (0, 1):
            xq, xx = dev(s, host(r.xs_q)[:, i]), dev(s, host(r.xs_xi)[:, i])
            o = s.mpc_measure(mask, V, xq, xx, xq.clone(), xx.clone(), d_P)
            assert (np.abs(host(d_P) - host(c.P_post)[:, i]) / scale).max() < 1e-9, (mask, i)
            assert np.abs(host(o["L"]) - host(c.L)[:, i]).max() < 1e-9, (mask, i)
            if i == 0:
                s.mpc_advance_estimated(d_eq, d_ex, d_P, W=W)


# 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("model", ["se3", "drone"])
def test_smallest_shapes_and_ragged_batches(model, N):
    """17 = a row group and a quarter; 67 = 16 waves and three quarters; 131: 3 B crosses a 256-thread block, and 2 B too.  Each
    trajectory's bits at B = 131 are its bits run alone."""
    mask = 0x5A5
    for B in (1, 5, 17, 67, 131):
        prob, q, xi, us = model_case(model, B, N=N)
        s = BatchedTrackingILQR(prob, B)
        check_measure(s, prob, np.asarray(q).reshape(B, 4, 4), xi, mask, seed=B, what="%s N=%d B=%d" % (model, N, B))
        r = held_policy(s, q, xi, us, "ms")
        check_advance_estimated(s, prob, r, seed=B, what="%s N=%d B=%d" % (model, N, B))
    # alone: the same inputs, row by row, on a handle of one trajectory
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    S0, W, V, _, _, _ = estimated_inputs(prob, B, seed=3)
    tq, tx, _ = scattered(prob, xq[:, 0], xx[:, 0], 4, 0.01, 0.01)
    rng = np.random.default_rng(5)
    w, n = rng.normal(size=(B, 6)) * 0.01, rng.normal(size=(B, 12)) * 0.005
    lb, ub = box_of(uu[:, 0], 6)

    def run(s1, rows):
        k = len(rows)
        d = [dev(s1, a[rows]) for a in (tq, tx, S0, xq[:, 0], xx[:, 0])]
        J = torch.zeros(k, dtype=torch.float64, device=s1.device)
        m = s1.mpc_measure(mask, V[rows], d[0], d[1], d[3], d[4], d[2], noise=n[rows])
        a = s1.mpc_advance_estimated(d[0], d[1], d[2], w=w[rows], W=W[rows], J_cl=J, u_lb=lb[rows], u_ub=ub[rows])
        return d + [J] + [m[k_] for k_ in ("L", "innov", "var_est")] + [a[k_] for k_ in ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi",
                                                                                             "us", "n_sat")]
    full = run(s, np.arange(B))
    for b in (0, 64, 130):
        s1 = BatchedTrackingILQR(prob, 1)
        s1.linearize_backward(xq[b:b + 1], xx[b:b + 1], uu[b:b + 1], ms=True)
        for x, y in zip(full, run(s1, np.array([b]))):
            assert same(x[b:b + 1], y), (model, N, b)


# 6 -------------------------------------------------------------------------------------------------------------------
def _loop(warm, mask=0x03F, **more):
    B, N, steps = 8, 40, 6
    prob, q, xi, pq, px, t0, noise, est = workloads.se3_mpc_estimated(B, steps, N=N, sigma_noise=0.02, seed=21)
    s = BatchedTrackingILQR(prob, B)
    seen = []
    res = s.mpc(q, xi, pq, px, steps, t0=t0, first_iters=10, iters_per_step=3, warm=warm, noise=noise, check_every=0, **ZERO,
                meas_mask=mask, **est, **more,
                on_step=lambda t, out: seen.append((t, host(out.xs_q).copy(), host(out.xs_xi).copy(), host(out.us).copy(),
                                                    host(out.J_hist).copy(), host(out.extra["est_P"]).copy())))
    assert [t for t, *_ in seen] == list(range(steps))
    assert (host(res.status) == _capi.ST_OK).all()
    # every solve began from the posterior and kept it: x*_0 of the step is the estimate, bit for bit (see posterior_held)
    for t, xs_q, xs_xi, *_ in seen:
        posterior_held(prob, xs_q[:, 0], xs_xi[:, 0], host(res.est_q)[:, t], host(res.est_xi)[:, t], (warm, t))
        assert np.abs(xs_q[:, 0] - host(res.xs_q)[:, t]).max() > 1e-6  # ... and not the true state
    return prob, (q, xi, pq, px, t0, noise, est), res, seen


def posterior_held(prob, x0_q, x0_xi, est_q, est_xi, what):
    """x*_0 = x0 to the bit.  The twist: the arrays are equal.  The pose: the workspace holds a unit quaternion and the [16]
    matrices of the C ABI go through it, matrix -> quaternion -> matrix, which is not the identity in the last bits (the same
    holds for any solve's xs_q[:, 0] against its x0_q); so the solve's xs_q[:, 0] must be the bits of that round trip of the
    posterior -- a solve of no iterations from it, in both modes -- and the matrices themselves agree to rounding."""
    assert np.array_equal(x0_xi, est_xi), what
    assert np.abs(x0_q - est_q).max() < 4e-15, (what, np.abs(x0_q - est_q).max())
    B = est_q.shape[0]
    s = BatchedTrackingILQR(prob, B)
    for mode in ("ms", "ss"):
        s.solve_begin(est_q, est_xi, np.zeros((B, prob.N, prob.m)), mode=mode, n_iterations=0, **ZERO)
        r = s.solve_end()
        assert same(r.xs_q[:, 0], x0_q) and same(r.xs_xi[:, 0], x0_xi), (what, mode)


def test_the_loop_step_by_step():
    """As check_loop does it, for every step from the device's own (x_true, est, P): the restatement's measure, the solve from the
    device's posterior, the advance."""
    mask, K0, K = 0x03F, 10, 3
    prob, (q, xi, pq, px, t0, noise, est), res, seen = _loop("controls", mask)
    B, N, steps = q.shape[0], prob.N, len(seen)
    rq, rx, ru, J = host(res.xs_q), host(res.xs_xi), host(res.us), host(res.J)
    eq, ex, ev, inn = host(res.est_q), host(res.est_xi), host(res.est_var), host(res.innov)
    Jcl = np.zeros(B)
    for b in range(B):
        tq0 = q[b] @ ob.se3_exp(est["est_dx0"][b, :6])
        assert np.abs(rq[b, 0] - tq0).max() < 1e-13 and np.abs(rx[b, 0] - (xi[b] + est["est_dx0"][b, 6:])).max() < 1e-13
        prior_q, prior_x, prior_P = q[b], xi[b], est["est_Sigma0"][b]
        for t in range(steps + 1):
            m = restate_measure(rq[b, t], rx[b, t], prior_q, prior_x, prior_P, mask, est["meas_V"][b], est["meas_noise"][b, t])
            scale = max(np.abs(prior_P).max(), 1e-300)
            assert np.abs(eq[b, t] - m["est_q"]).max() < 1e-10 and np.abs(ex[b, t] - m["est_xi"]).max() < 1e-10, (b, t)
            assert np.abs(inn[b, t] - m["innov"]).max() < 1e-10 and np.abs(ev[b, t] - m["var_est"]).max() < 1e-9 * scale, (b, t)
            if t == steps:
                break
            _, xs_q, xs_xi, us, Jh, gP = seen[t]
            assert np.abs(gP[b] - m["P"]).max() < 1e-9 * scale and np.array_equal(gP[b], gP[b].T), (b, t)
            assert np.array_equal(ev[b, t], np.diag(gP[b])) and np.array_equal(ru[b, t], us[b, 0])
            op = window_problem(prob, pq[b], px[b], int(t0[b]), t)
            us_in = np.zeros((N, prob.m)) if t == 0 else mpc_shift(seen[t - 1][1][b][None], seen[t - 1][3][b][None],
                                                                   eq[b, t][None], eq[b, t][None])[1][0]
            o = restate_mpc_step(op, eq[b, t], ex[b, t], us_in, K0 if t == 0 else K)
            assert np.abs(Jh[b] / o["J_hist"] - 1).max() < 1e-9, (t, b)
            assert np.abs(us[b] - o["us"]).max() / np.abs(o["us"]).max() < 1e-6, (t, b)
            a = restate_advance_estimated(op, xs_q[b], xs_xi[b], us[b], rq[b, t], rx[b, t], gP[b], noise[b, t], est["est_W"][b])
            assert rel(rq[b, t + 1], a["x_true_q"]) < 1e-13 and rel(rx[b, t + 1], a["x_true_xi"]) < 1e-13, (b, t)
            Jcl[b] += a["dJ"]
            prior_q, prior_x, prior_P = a["x_next_q"], a["x_next_xi"], a["P"]
    assert rel(J, Jcl) < 1e-12
    assert (host(res.iters)[:, 0] == K0).all() and (host(res.iters)[:, 1:] == K).all()


def test_the_loop_with_warm_states():
    prob, _, res, seen = _loop("states")
    for k in ("xs_q", "xs_xi", "us", "J", "est_q", "est_xi", "est_var", "innov"):
        assert np.isfinite(host(getattr(res, k))).all(), k
    assert (host(res.est_var) > 0).all() and host(res.innov)[..., :6].any() and not host(res.innov)[..., 6:].any()


def test_the_loop_reports_the_true_states_under_a_sphere_and_a_box():
    """The planner keeps out of a sphere on the estimate; the report is on the TRUE states: clearance recomputed on the host from
    res.xs_q, which is not the clearance of the estimates."""
    B, N, steps = 8, 40, 6
    prob, q, xi, pq, px, t0, noise, est = workloads.se3_mpc_estimated(B, steps, N=N, sigma_noise=0.02, seed=21)
    c = pq[np.arange(B), t0 + 4, :3, 3] + np.array([0.05, 0.0, 0.0])
    obs = np.concatenate([c, np.full((B, 1), 0.1)], axis=1)[:, None, :]
    s = BatchedTrackingILQR(prob, B)
    res = s.mpc(q, xi, pq, px, steps, t0=t0, first_iters=6, iters_per_step=2, noise=noise, **ZERO, obstacles=obs,
                u_lb=-np.full(6, 2.0), u_ub=np.full(6, 2.0), meas_mask=0x03F, **est)
    assert res.n_sat is not None and res.max_violation is not None and np.isfinite(host(res.xs_q)).all()
    d_true = np.linalg.norm(host(res.xs_q)[:, :, :3, 3] - obs[:, :, :3], axis=-1) - obs[:, :, 3]
    d_est = np.linalg.norm(host(res.est_q)[:, :, :3, 3] - obs[:, :, :3], axis=-1) - obs[:, :, 3]
    assert np.abs(host(res.clearance) - d_true).max() < 1e-12
    assert np.abs(host(res.clearance) - d_est).max() > 1e-6
    assert (np.abs(host(res.us)) <= 2.0).all()


# 7 -------------------------------------------------------------------------------------------------------------------
def test_the_filter_does_its_job():
    """One problem replicated over 256 trajectories with seeded noise per trajectory (tests/mpc_estimated.py::filter_case, the
    inputs tests/test_mpc_estimated_cpu.py passes on the restatement alone with a factor two to spare): the RMS position error
    of the posterior over the last six steps is below the sensor's own deviation and below that of the same run without a
    sensor; per coordinate the sample variance of x_true (-) est at the last step lies within MC_MULT standard errors of the
    mean est_var."""
    c = filter_case()
    runs = {}
    for name in ("on", "off"):
        kw = dict(c["kw"])
        if name == "off":
            kw.update(meas_mask=0, meas_V=None)
        r = BatchedTrackingILQR(c["prob"], c["args"][0].shape[0]).mpc(*c["args"], **kw)
        assert (host(r.status) == _capi.ST_OK).all()
        runs[name] = tuple(host(getattr(r, k)) for k in ("xs_q", "xs_xi", "est_q", "est_xi", "est_var"))
    fig = filter_figures(c["V"], runs["on"], runs["off"])
    print(fig)
    for k, v in fig.items():
        assert v < 1.0, (k, v)


# 8 -------------------------------------------------------------------------------------------------------------------
class Raw:
    """The two entry points raw through _capi on buffers of B rows; every argument can be replaced (None: NULL)."""

    def __init__(self, s, B):
        f64 = dict(dtype=torch.float64, device=s.device)
        g = torch.Generator(device="cpu").manual_seed(B)
        rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64).to(s.device)  # noqa: E731
        eye = torch.eye(4, **f64).reshape(16)
        self.s, self.B = s, B
        self.b = dict(V=rnd(B, 12) + 0.5, x_q=eye.repeat(B, 1), x_xi=rnd(B, 6), n=0.01 * rnd(B, 12), est_q=eye.repeat(B, 1),
                      est_xi=rnd(B, 6), P=torch.eye(12, **f64).repeat(B, 1, 1) * 0.01, L=rnd(B, 12, 12), innov=rnd(B, 12),
                      var_est=rnd(B, 12), w=0.01 * rnd(B, 6), lb=-rnd(B, s.m), ub=rnd(B, s.m), W=torch.eye(6, **f64).repeat(B, 1, 1) * 1e-4,
                      xn_q=rnd(B, 16), xn_xi=rnd(B, 6), u=rnd(B, s.m), xs_q=rnd(B, s.N + 1, 16), xs_xi=rnd(B, s.N + 1, 6),
                      us=rnd(B, s.N, s.m), J=rnd(B), n_sat=torch.full((B,), 7, dtype=torch.int32, device=s.device))

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in self.b.items()}

    def unchanged(self, snap):
        torch.cuda.synchronize()
        return all(torch.equal(v, snap[k]) for k, v in self.b.items())

    def _p(self, names, kw):
        return [C.c_void_p(0 if kw.get(k, 1) is None else self.b[k].data_ptr()) for k in names]

    def measure(self, B=None, mask=0x03F, **kw):
        rc = self.s.lib.tolg_mpc_measure(self.s._h, self.B if B is None else B, mask,
                                         *self._p(("V", "x_q", "x_xi", "n", "est_q", "est_xi", "P", "L", "innov", "var_est"), kw),
                                         self.s._stream())
        torch.cuda.synchronize()
        return rc

    def advance(self, B=None, **kw):
        rc = self.s.lib.tolg_mpc_advance_estimated(self.s._h, self.B if B is None else B,
                                                   *self._p(("w", "lb", "ub", "x_q", "x_xi", "P", "W", "xn_q", "xn_xi", "u", "xs_q",
                                                             "xs_xi", "us", "J", "n_sat"), kw), self.s._stream())
        torch.cuda.synchronize()
        return rc


def test_argument_rules_raw():
    B = 4
    prob, q, xi, us = workloads.se3_tracking(B, N=20)
    s = BatchedTrackingILQR(prob, B)
    r = Raw(s, B)
    snap = r.snapshot()
    # measure: every TOLG_E_ARG; a refused call changes nothing
    assert r.measure(B=0) == -1 and r.measure(B=B + 1) == -1 and r.measure(mask=0x1000) == -1 and r.measure(mask=-1) == -1
    assert r.measure(V=None) == -1
    for k in ("x_q", "x_xi", "est_q", "est_xi", "P"):
        assert r.measure(**{k: None}) == -1, k
    # advance: no held policy yet
    assert r.advance() == -1
    assert r.unchanged(snap)
    # measure needs no held policy, takes NULL outputs, NULL noise and, with nothing measured, a NULL V
    assert r.measure() == 0 and r.measure(L=None, innov=None, var_est=None, n=None) == 0 and r.measure(mask=0, V=None) == 0
    assert r.measure(B=B - 1) == 0  # any batch up to max_batch
    # ... and is legal during a solve in flight, which it does not disturb: the bits of an undisturbed solve
    ref = BatchedTrackingILQR(prob, B).fit_batch(q, xi, us, mode="ms", **KW)
    s.solve_begin(q, xi, us, mode="ms", **KW)
    s.solve_iterate(2)
    snap = r.snapshot()
    assert r.advance() == -1 and r.unchanged(snap)  # a solve in flight: no policy to advance
    assert r.measure() == 0
    s.solve_iterate(2)
    out = s.solve_end()
    assert same(out.xs_q, ref.xs_q) and same(out.us, ref.us) and same(out.J_hist, ref.J_hist)
    # advance: every TOLG_E_ARG on a held policy
    snap = r.snapshot()
    assert r.advance(B=B - 1) == -1 and r.advance(B=0) == -1
    assert r.advance(lb=None) == -1 and r.advance(ub=None) == -1  # exactly one bound
    for k in ("x_q", "x_xi", "P", "xs_q", "xs_xi", "us"):
        assert r.advance(**{k: None}) == -1, k
    assert r.unchanged(snap)
    assert r.advance() == 0 and r.advance(lb=None, ub=None) == 0
    assert r.advance(w=None, W=None, xn_q=None, xn_xi=None, u=None, J=None, n_sat=None) == 0
    assert r.advance(lb=None, ub=None) == 0 and not host(r.b["n_sat"]).any()  # no box moves nothing
    # the binding: the host checks come before the device
    f64 = dict(dtype=torch.float64, device=s.device)
    good = dict(x_true_q=r.b["x_q"].clone(), x_true_xi=r.b["x_xi"].clone(), P=r.b["P"].clone())
    for bad in (dict(P=host(good["P"])), dict(P=torch.zeros(B, 12, 11, **f64)), dict(x_true_xi=torch.zeros(B + 1, 6, **f64)),
                dict(u_lb=np.zeros(6)), dict(W=-np.eye(6)), dict(w=np.zeros((B, 5))), dict(x_true_q=good["x_true_q"].float())):
        with pytest.raises(ValueError):
            s.mpc_advance_estimated(**{**good, **bad})
    with pytest.raises(ValueError, match="out of scope"):
        s.mpc(q, xi, np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy(),
              np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape).copy(), 2, meas_mask=0, act_tau=0.02)


def test_the_so3_mask_rule():
    for model in ("so3", "pendulum"):
        B = 3
        prob, q, xi, us = model_case(model, B)
        r = Raw(BatchedTrackingILQR(prob, B), B)
        snap = r.snapshot()
        for mask in (0x008, 0x020, 0x200, 0x800, 0x03F):
            assert r.measure(mask=mask) == -1, (model, mask)
        assert r.unchanged(snap)
        assert r.measure(mask=0x1C7) == 0 and r.measure(mask=0) == 0
