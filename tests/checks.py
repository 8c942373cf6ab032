"""Assertion-bearing checks that more than one test module calls, each with the tolerances of the test it came from."""
import warnings

import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import mpc_shift
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_constraints import SphereObstacleConstraint
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_controller import (iLQR_Tracking_SE3,
                                                                                           iLQR_Tracking_SE3_MS)
from trajectory_optimization_matrix_lie_groups_amd.traoptlibrary.traopt_cost import ALConstrainedCost
from tests.restate import MyCost, MyDynamics, restate_mpc_step, restate_policy, window_problem
from tests.limits import near_bound, restate_limited_batch
from tests.support import (EXP_TIERS, LOG_TIERS, assert_coverage, determined, nudged, policy_rollout_tags, sample_spread)
from tests.support import ZERO, host, problem_of_kind, random_traj_embedded, rel, same


K1_FIELDS = ("Fx", "d", "lx", "lxx11", "J")   # what the linearisation alone produces (the sweep's K, k, grad, mu_delta follow)


def check_linearize_backward(prob, xs_q, xs_xi, us, ms, solver=None, fields=None, bounds=None):
    """K1 + K2 (tolg_linearize_backward) on the given trajectories against the oracle's _linearization/_backward_pass,
    trajectory by trajectory; solver: a handle on prob (default: a fresh one of the batch's size).  fields: the subset to
    compare (default: all of Fx, d, lx, lxx11, J, K, k, grad, mu_delta).  bounds: {field: [B] or scalar} in place of a
    field's bound below, for trajectories on which the reference itself is known to be further from exact than that.
    Returns the worst figure per field."""
    B = xs_q.shape[0]
    solver = BatchedTrackingILQR(prob, B) if solver is None else solver
    r = solver.linearize_backward(xs_q, xs_xi, us, ms=ms)
    torch.cuda.synchronize()
    op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref,
                          pend_mass=prob.pend_mass, pend_length=prob.pend_length)
    want = lambda f: fields is None or f in fields  # noqa: E731
    worst = {}

    def bound(f, b, default):
        v = default if bounds is None or f not in bounds else bounds[f]
        return float(v[b]) if np.ndim(v) else float(v)

    def within(f, b, err, default):
        worst[f] = max(worst.get(f, 0.0), float(err))
        assert err < bound(f, b, default), (f, b, float(err), bound(f, b, default))

    for b in range(B):
        o = ob.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=ms)
        if want("Fx"):
            within("Fx", b, rel(r["Fx"][b].cpu(), o["Fx"]), 1e-12)
        if want("d"):
            within("d", b, np.abs(r["d"][b].cpu().numpy() - o["d"]).max() / max(1.0, np.abs(o["d"]).max()), 1e-11)
        if want("lx"):
            within("lx", b, rel(r["lx"][b].cpu(), o["Lx"]), 1e-11)
        if want("lxx11"):
            within("lxx11", b, rel(r["lxx11"][b].cpu(), o["Lxx"][:, :6, :6]), 1e-11)
        if want("J"):
            assert float(r["J"][b]) == pytest.approx(o["J"], rel=bound("J", b, 1e-12))
            worst["J"] = max(worst.get("J", 0.0), abs(float(r["J"][b]) / o["J"] - 1))
        if want("K"):
            within("K", b, rel(r["K"][b].cpu(), o["K"]), 1e-8)
        if want("k"):
            within("k", b, rel(r["k"][b].cpu(), o["k"]), 1e-8)
        if want("grad"):
            assert float(r["grad"][b]) == pytest.approx(o["grad"], rel=1e-9)
        if want("mu_delta"):
            assert float(r["mu_delta"][b, 0]) == o["mu"] and float(r["mu_delta"][b, 1]) == o["delta"]
    return worst


def al_oracle(prob, x0_q, x0_xi, us0, lb, ub, n_al, n_ilqr, tol_constr, mu0=1e-2, mu_scale=10.0, mu_max=1e8):
    """AL_iLQR_Tracking_SE3_MS.fit restated with the oracle as inner solver
    (reference traoptlibrary/traopt_controller.py:3218-3293; the reference class itself does not
    run at HEAD -- SURVEY App. C-Q7 -- so this is the specification: parity unpinned)."""
    N, m = prob.N, prob.m
    lam = np.zeros((N, 2 * m)); imu = np.full((N, 2 * m), mu0); mu = mu0
    for it in range(n_al):
        op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref,
                              al=dict(lb=lb, ub=ub, lam=lam, imu=imu))
        o = ob.fit(op, x0_q, x0_xi, us0, mode="ms", max_iter=n_ilqr, tol_grad=1e-6, tol_defect=1e-6)
        g = np.concatenate([lb[None] - o["us"], o["us"] - ub[None]], axis=1)
        if max(g.max(), 0.0) < tol_constr:
            return o, lam, imu, mu, it + 1
        mu_new = min(mu * mu_scale, mu_max)
        lam_new = np.clip(lam + imu * g, 0.0, None)
        imu = np.where((g < 0.0) & (lam_new == 0.0), 0.0, mu_new)
        lam, mu = lam_new, mu_new
    return o, lam, imu, mu, n_al


def check_ring_against_statement(kind, B, N, spread):
    """The body of test_ring_kernel_matches_statement_kernel_on_random_trajectories (tests/test_gpu_expected_change.py), for
    any kind / batch / horizon / spread."""
    prob, *_ = problem_of_kind(kind, 1, N)
    xs_q, xs_xi, us = random_traj_embedded(prob, B, seed=3 + N, spread=spread)
    if B >= 5:  # two trajectories with rotation defects near pi: candidates for the hand-back
        wild, _, _ = random_traj_embedded(prob, B, seed=4 + N, spread=1.6)
        xs_q[1], xs_q[4] = wild[1], wild[4]
    solver = BatchedTrackingILQR(prob, B)
    solver.linearize_backward(xs_q, xs_xi, us, ms=True)
    es, _ = solver.expected_change(B, "statement")
    er, flag = solver.expected_change(B, "ring")
    er2, flag2 = solver.expected_change(B, "ring")
    ea, _ = solver.expected_change(B, "auto")
    torch.cuda.synchronize()
    es, er, er2, ea, flag, flag2 = (t.cpu().numpy() for t in (es, er, er2, ea, flag, flag2))
    np.testing.assert_array_equal(flag, flag2)
    np.testing.assert_array_equal(er, er2)
    keep = flag == 0
    assert keep.sum() >= B // 2
    assert np.isfinite(es).all()
    scale = np.abs(es).max(axis=1, keepdims=True)
    assert (np.abs(er[keep] - es[keep]) / scale[keep]).max() < 1e-11
    assert np.isnan(er[~keep]).all()
    np.testing.assert_array_equal(ea[~keep], es[~keep])
    np.testing.assert_array_equal(ea[keep], er[keep])


_TOL = {"J_hist": 1e-11, "xs_q": 1e-9, "xs_xi": 1e-9, "us": 1e-9, "mu_hist": 0.0}


def assert_same(keep, rs):
    for k, v in keep.items():
        w = getattr(rs, k)
        if not v.dtype.is_floating_point:
            assert torch.equal(v, w), k
            continue
        assert torch.equal(torch.isnan(v), torch.isnan(w)), k  # untouched history entries are NaN on both sides
        a = torch.nan_to_num(v, nan=0.0).cpu().numpy(); b = torch.nan_to_num(w, nan=0.0).cpu().numpy()
        if k in ("grad_hist", "defect_hist"):  # rounding-level quantities once converged: absolute floor
            assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max() + 1e-11, (k, np.abs(a - b).max())
        else:
            assert rel(a, b) <= _TOL[k], (k, rel(a, b))


def check_advance(s, r, ops, w):
    B, N = r.us.shape[0], s.N
    J1 = torch.zeros(B, dtype=torch.float64, device=s.device)
    a = s.mpc_advance(w, J_cl=J1)
    xq, xx, uu = host(r.xs_q), host(r.xs_xi), host(r.us)
    fin = [b for b in range(B) if np.isfinite(xq[b]).all() and np.isfinite(xx[b]).all() and np.isfinite(uu[b]).all()]
    assert len(fin) >= B // 2
    for b in fin:
        op = ops[b]
        q1, x1 = ob.f(op, xq[b, 0], xx[b, 0], uu[b, 0])
        assert rel(host(a["x_next_q"])[b], q1) < 1e-13 and rel(host(a["x_next_xi"])[b], x1 + w[b]) < 1e-13
        qN, xN = ob.f(op, xq[b, N], xx[b, N], uu[b, N - 1])
        assert rel(host(a["xs_q"])[b, N], qN) < 1e-13 and rel(host(a["xs_xi"])[b, N], xN) < 1e-13
        assert abs(host(J1)[b] / ob.cost(op, xq[b, 0], xx[b, 0], uu[b, 0], 0)[0] - 1) < 1e-12
    # the shift: bitwise the host shift of solve_end's output
    sq, su = mpc_shift(xq, uu, host(a["x_next_q"]), host(a["xs_q"])[:, N])
    sx, _ = mpc_shift(xx, uu, host(a["x_next_xi"]), host(a["xs_xi"])[:, N])
    for k, shifted in (("xs_q", sq), ("xs_xi", sx), ("us", su)):
        diff = ~np.equal(host(a[k]), shifted) & ~(np.isnan(host(a[k])) & np.isnan(shifted))
        assert not diff.any(), (k, sorted(set(zip(*np.nonzero(diff)[:2])))[:10])
    assert same(a["u"], uu[:, 0])
    # twice: the same bits, the policy untouched (J_cl accumulates)
    b2 = s.mpc_advance(w, J_cl=J1)
    for k in ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us"):
        assert same(a[k], b2[k]), k
    assert rel(host(J1)[fin], 2 * np.array([ob.cost(ops[b], xq[b, 0], xx[b, 0], uu[b, 0], 0)[0] for b in fin])) < 1e-12


def check_loop(B, N, steps, K0, K):
    """mpc() on se3_mpc's paths against restate_mpc_step, step by step: every window's solve, the applied input, the
    closed-loop state and cost."""
    prob, q, xi, pq, px, t0, noise = workloads.se3_mpc(B, steps, N=N, sigma_noise=0.02, seed=21)
    s = BatchedTrackingILQR(prob, B)
    seen = []
    r = s.mpc(q, xi, pq, px, steps, t0=t0, first_iters=K0, iters_per_step=K, warm="controls", noise=noise, check_every=0,
              **ZERO, on_step=lambda t, out: seen.append((t, host(out.xs_q).copy(), host(out.xs_xi).copy(), host(out.us).copy(),
                                                  host(out.J_hist).copy())))
    assert [t for t, *_ in seen] == list(range(steps))
    rq, rx, ru, J = host(r.xs_q), host(r.xs_xi), host(r.us), host(r.J)
    assert np.array_equal(rq[:, 0], q) and np.array_equal(rx[:, 0], xi)
    Jcl = np.zeros(B)
    for t, xs_q, xs_xi, us, Jh in seen:
        us_in = np.zeros((B, N, prob.m)) if t == 0 else mpc_shift(seen[t - 1][1], seen[t - 1][3], rq[:, t], rq[:, t])[1]
        assert np.array_equal(ru[:, t], us[:, 0])  # the applied input is the step's u*_0
        for b in range(B):
            op = window_problem(prob, pq[b], px[b], int(t0[b]), t)
            o = restate_mpc_step(op, rq[b, t], rx[b, t], us_in[b], K0 if t == 0 else K)
            assert np.abs(Jh[b] / o["J_hist"] - 1).max() < 1e-9, (t, b)
            assert np.abs(us[b] - o["us"]).max() / np.abs(o["us"]).max() < 1e-6, (t, b)
            # the closed-loop state is the advance's x_next: f(x*_0, u*_0) + noise
            q1, x1 = ob.f(op, xs_q[b, 0], xs_xi[b, 0], us[b, 0])
            assert rel(rq[b, t + 1], q1) < 1e-13 and rel(rx[b, t + 1], x1 + noise[b, t]) < 1e-13
            Jcl[b] += ob.cost(op, xs_q[b, 0], xs_xi[b, 0], us[b, 0], 0)[0]
    assert rel(J, Jcl) < 1e-12
    assert (host(r.status) == _capi.ST_OK).all()
    assert (host(r.iters)[:, 0] == K0).all() and (host(r.iters)[:, 1:] == K).all()


def host_solve(prob, x0_q, x0_xi, us0, obs, lam, imu, kw, states=False):
    """The mirror's host generic path with fixed sphere multipliers: (J per iteration, us[, xs]).  states: xs as well."""
    op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
    c = SphereObstacleConstraint(obs[:, :3], obs[:, 3])
    al = ALConstrainedCost(MyCost(op, prob.m), c, prob.N)
    al.lmbd = lam.copy()
    al.Imu = np.stack([np.diag(d) for d in imu])
    ms = kw["mode"] == "ms"
    J = []

    def cb(*a):
        a[-5 if ms else -3].append(a[3])
        J.append(a[3])

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rollout = kw.get("rollout", "nonlinear")
        if ms:
            ctl = iLQR_Tracking_SE3_MS(MyDynamics(op, prob.m), al, prob.N, prob.q_ref, prob.xi_ref, rollout=rollout,
                                       line_search=kw.get("line_search", False))
        else:
            ctl = iLQR_Tracking_SE3(MyDynamics(op, prob.m), al, prob.N, rollout=rollout)
        xs, us, *_ = ctl.fit([x0_q, x0_xi], us0, n_iterations=kw["n_iterations"], tol_grad_norm=0.0, on_iteration=cb)
    return (np.array(J), us, xs) if states else (np.array(J), us)


def update_restated(g, lam, imu, mu, mu_scale=10.0):
    mu_new = mu * mu_scale
    ln = np.maximum(0.0, lam + imu * g)
    return ln, np.where((g < 0) & (ln == 0), 0.0, mu_new)


def check_restatement(s, r, ops, dx0, w, min_finite=None):
    """min_finite: the share of samples the restatement must keep finite, as (numerator, denominator); default a half."""
    g = s.gains()
    p = s.policy_rollout(dx0, w, trajectories=True)
    K = host(g["K"])
    S = dx0.shape[1]
    ok = 0
    for b, op in enumerate(ops):
        J, xq, xx, uu = restate_policy(op, host(r.xs_q)[b], host(r.xs_xi)[b], host(r.us)[b], K[b], dx0[b], w[b], S)
        fin = np.isfinite(J)  # a sample the CPU sees diverge must diverge on the device, and be flagged there
        assert np.array_equal(host(p.status)[b], np.where(fin, _capi.ST_OK, _capi.ST_NONFINITE))
        assert np.abs(host(p.xs_q)[b][fin] - xq[fin]).max(initial=0) < 1e-10
        assert np.abs(host(p.xs_xi)[b][fin] - xx[fin]).max(initial=0) < 1e-10
        assert np.abs(host(p.us)[b][fin] - uu[fin]).max(initial=0) < 1e-8
        assert np.abs(host(p.J)[b][fin] / J[fin] - 1).max(initial=0) < 1e-9
        ok += int(fin.sum())
    num, den = (1, 2) if min_finite is None else min_finite
    assert ok >= len(ops) * S * num // den, (ok, len(ops) * S)


# the limited closed loops (tolg_policy_rollout_limited) against tests/limits.py::restate_policy_limited
def limited_conditions(R, lb, ub):
    """The conditions a parity case must meet, on the restatement alone.  Returns (finite [B, S], near a bound [B, S])."""
    fin = np.array([np.isfinite(r["J"]) for r in R])
    ns = np.array([r["n_sat"] for r in R])
    near = np.array([near_bound(r["uc"], lb[b], ub[b]) for b, r in enumerate(R)]) & fin
    nf = int(fin.sum())
    print("restatement: finite %d of %d, saturated %d, free %d, near a bound %d"
          % (nf, fin.size, int((ns[fin] > 0).sum()), int((ns[fin] == 0).sum()), int(near.sum())))
    assert nf >= fin.size // 2
    assert 4 * int((ns[fin] > 0).sum()) >= nf
    assert (ns[fin] == 0).any()
    assert 4 * int(near.sum()) <= nf
    return fin, near


def compare_limited(p, R, fin, near, keep=None):
    """keep [B, S] (default: all): the samples whose values are compared; the status of every sample is."""
    worst = dict(xs_q=0.0, xs_xi=0.0, us=0.0, J=0.0, u_excess=0.0)
    if keep is not None:
        fin, full = fin & keep, fin
    for b, r in enumerate(R):
        f = fin[b]
        assert np.array_equal(host(p.status)[b], np.where(f if keep is None else full[b], _capi.ST_OK, _capi.ST_NONFINITE))
        worst["xs_q"] = max(worst["xs_q"], np.abs(host(p.xs_q)[b][f] - r["xs_q"][f]).max(initial=0))
        worst["xs_xi"] = max(worst["xs_xi"], np.abs(host(p.xs_xi)[b][f] - r["xs_xi"][f]).max(initial=0))
        worst["us"] = max(worst["us"], np.abs(host(p.us)[b][f] - r["us"][f]).max(initial=0))
        worst["J"] = max(worst["J"], np.abs(host(p.J)[b][f] / r["J"][f] - 1).max(initial=0))
        worst["u_excess"] = max(worst["u_excess"], np.abs(host(p.u_excess)[b][f] - r["u_excess"][f]).max(initial=0))
    print("device against restatement:", worst)
    assert worst["xs_q"] < 1e-10 and worst["xs_xi"] < 1e-10 and worst["us"] < 1e-8 and worst["J"] < 1e-9   # check_restatement's
    assert worst["u_excess"] < 1e-8
    for b, r in enumerate(R):
        exact = fin[b] & ~near[b]
        assert np.array_equal(host(p.n_sat)[b][exact], r["n_sat"][exact]), b
    return worst


def compare_estimated(p, R, keep):
    """tolg_policy_rollout_estimated's outputs p (trajectories and estimates asked for) against the restatement R
    (tests/estimated.py::restate_estimated_batch), at check_restatement's bounds: the status of every sample, the values of the
    samples in keep [B, S] that are finite.  Returns the worst figure per field."""
    worst = dict(xs_q=0.0, xs_xi=0.0, est_q=0.0, est_xi=0.0, us=0.0, J=0.0)
    for b, r in enumerate(R):
        fin = np.isfinite(r["J"])  # a sample the CPU sees diverge must diverge on the device, and be flagged there
        assert np.array_equal(host(p.status)[b], np.where(fin, _capi.ST_OK, _capi.ST_NONFINITE)), b
        fin = fin & keep[b]
        for name, tol in (("xs_q", 1e-10), ("xs_xi", 1e-10), ("est_q", 1e-10), ("est_xi", 1e-10), ("us", 1e-8)):
            e = np.abs(host(getattr(p, name))[b][fin] - r[name][fin]).max(initial=0)
            worst[name] = max(worst[name], float(e))
            assert e < tol, (b, name, e)
        e = np.abs(host(p.J)[b][fin] / r["J"][fin] - 1).max(initial=0)
        worst["J"] = max(worst["J"], float(e))
        assert e < 1e-9, (b, "J", e)
    return worst


def limited_guard(op, prob, nom, K, dx0, w, widen):
    """The conditions and the coverage guard of the limited loop at large rotations, on the restatement alone: the box from
    the unlimited restatement, limited_conditions under it, the Log tier of every start deviation and the Exp tier of every
    knot's twist as test (d) of tests/test_gpu_large_rotation.py counts them, and the samples the restatement determines
    (tests/support.py::determined, the gains moved in their last place): three quarters at least, with the same n_sat.
    Returns (lb, ub, the restatement, keep [B, S], the spread per field [B, S])."""
    B = dx0.shape[0]
    lb, ub, R = restate_limited_batch([op] * B, nom, K, dx0, w, widen=widen)
    limited_conditions(R, lb, ub)
    tags = [t for b, r in enumerate(R) for t in policy_rollout_tags(prob, nom.xs_q[b, 0], r["xs_q"], r["xs_xi"])]
    assert_coverage(tags, need=LOG_TIERS + EXP_TIERS[1:])
    _, _, R2 = restate_limited_batch([op] * B, nom, nudged(K, np.random.default_rng(5)), dx0, w, box=(lb, ub))
    sp = sample_spread(R, R2)
    keep = determined(sp) & np.array([a["n_sat"] == b["n_sat"] for a, b in zip(R, R2)])
    assert 4 * int(keep.sum()) >= 3 * keep.size, (int(keep.sum()), keep.size)
    return lb, ub, R, keep, sp
