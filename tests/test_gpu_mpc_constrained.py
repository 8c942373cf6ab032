"""Constrained receding-horizon MPC: the planner inside mpc() under an input box and keep-out spheres.

1. tolg_al_mpc_step against the NumPy restatement of tests/mpc_al.py: every shape at which the kernel takes another path,
   box / spheres / both, static and moving geometry, the in-place shift bitwise, sentinels, repeatability, and against
   tolg_al_update_state where both apply;
2. tolg_set_al_obstacle_windows: the packed bits of tolg_set_al_obstacles_moving on host-sliced windows, argument errors;
3. mpc(...) is its parts: the same loop written from the public methods, bitwise; batch independence;
4. with mu0 = 0 the constrained loop gives the bits of the unconstrained one;
5. it does something: less penetration, less saturation;
6. the handle's state behind mpc(), and the argument errors;
7. full size once."""
import ctypes as C

import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import mpc_window_index
from tests.mpc_al import al_mpc_step_restated, g_box, g_spheres, shifted
from tests.support import ZERO, assert_bitwise, bits, host, same

pytestmark = pytest.mark.gpu
f64 = dict(dtype=torch.float64, device="cuda:0")
P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731

TILE = 512            # AL_STEP_TILE (csrc/tolg_kernels.hip): the doubles of one multiplier set a workgroup moves per tile
N_LONG = 2 * TILE + 2  # K = 1: N + 1 sphere rows = two tiles plus three rows; every other row width: more tiles still
SENTINEL = -7.25
RT, AT = 1e-12, 1e-15  # test_outer_update_against_a_restatement's tolerances (tests/test_gpu_obstacles.py)


def _problem(kind, N):
    """A problem of N knots for the step kernel, which reads N, m and the kind alone"""
    base = (workloads.drone_tracking if kind == "drone" else workloads.se3_tracking)(1, N=20)[0]
    return TrackingProblem(base.kind, base.J, base.dt, base.Q, base.R, base.P, np.tile(np.eye(4), (N + 1, 1, 1)),
                           np.zeros((N + 1, 6)))


def _step_inputs(N, m, B, K, moving, sat, seed):
    """Controls on both sides of a box, positions scattered about the surfaces of the spheres (0.5 .. 1.5 radii from a centre),
    so that g has both signs; the trajectories `sat` satisfy everything: inside the box, far from every sphere."""
    rng = np.random.default_rng(seed)
    lb, ub = -rng.uniform(0.5, 1.5, m), rng.uniform(0.5, 1.5, m)
    us = rng.normal(size=(B, N, m))
    pos = rng.normal(size=(B, N + 1, 3))
    d = rng.normal(size=(B, N + 1, K, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    r = rng.uniform(0.2, 0.6, (B, N + 1, K))
    obs = np.concatenate([pos[:, :, None] + d * (r * rng.uniform(0.5, 1.5, (B, N + 1, K)))[..., None], r[..., None]], axis=-1)
    if not moving:  # one geometry for every knot: knot i sits at the surface of sphere i % K of knot 0's field
        obs = np.ascontiguousarray(obs[:, 0])
        k = np.arange(N + 1) % K
        dd = rng.normal(size=(B, N + 1, 3))
        dd /= np.linalg.norm(dd, axis=-1, keepdims=True)
        pos = obs[:, k, :3] + dd * (obs[:, k, 3] * rng.uniform(0.5, 1.5, (B, N + 1)))[..., None]
    # every other trajectory violates both: an input beyond the box, the last knot half a radius from a centre
    us[:, 0, 0] = ub[0] + 0.5
    last = obs[:, N, 0] if moving else obs[:, 0]
    pos[:, N] = last[:, :3] + 0.5 * last[:, 3:] * d[:, N, 0]
    for b in sat:
        us[b] = np.clip(us[b], 0.9 * lb, 0.9 * ub)
        pos[b] += 1000.0
    xs_q = np.tile(np.eye(4), (B, N + 1, 1, 1))
    xs_q[..., :3, 3] = pos
    return lb, ub, us, xs_q, obs


def _mults(rng, B, rows, W):
    """Random multipliers with some I_mu = 0 and some lambda = 0, as views between two sentinel trajectories"""
    out = []
    for hi in (1.0, 20.0):
        a = rng.uniform(0.0, hi, (B, rows, W)) * (rng.uniform(size=(B, rows, W)) > 0.3)
        buf = torch.full((B + 2, rows, W), SENTINEL, **f64)
        buf[1:B + 1] = torch.as_tensor(a, **f64)
        out.append(buf)
    return out


def _run_step(s, B, xs_q, us, mu0, shift, box, sph, tol=1e-2, mu_scale=10.0, mu_max=1e8):
    """One tolg_al_mpc_step on fresh copies of the multiplier buffers (box, sph: [lam_buf, imu_buf] or None; sph also holds
    the geometry).  Returns (maxviol, mu, box views, sphere views, the buffers)."""
    bufs = [None if x is None else [x[0].clone(), x[1].clone()] for x in (box, sph)]
    view = lambda x: None if x is None else (x[0][1:B + 1], x[1][1:B + 1])  # noqa: E731
    vb, vs = view(bufs[0]), view(bufs[1])
    if box is not None:
        s.set_al(box[2], box[3], *vb)
    if sph is not None:
        s.set_al_obstacles(sph[2], *vs)
    mu = torch.full((B,), mu0, **f64)
    mv = s.al_mpc_step(xs_q if sph is not None else None, us if box is not None else None, mu, mu_scale, mu_max, tol, shift)
    s.set_al(None)
    s.set_al_obstacles(None)
    return mv, mu, vb, vs, bufs


@pytest.mark.parametrize("N", [1, 2, 7, 40, N_LONG])
@pytest.mark.parametrize("kind", ["se3", "drone"])
def test_step_against_the_restatement(kind, N):
    prob = _problem(kind, N)
    m, mu0, tol = prob.m, 0.5, 1e-2
    seed = 0
    for B in (1, 5, 13):
        s = BatchedTrackingILQR(prob, B)
        for K in (1, 3, 16):
            for case in ("box", "static", "moving", "box+static", "box+moving"):
                for sat in ([[], [0]] if B == 1 else [[B - 1]]):
                    seed += 1
                    rng = np.random.default_rng(1000 + seed)
                    lb, ub, us, xs_q, obs = _step_inputs(N, m, B, K, "moving" in case, sat, seed)
                    box = _mults(rng, B, N, 2 * m) + [lb, ub] if "box" in case else None
                    sph = _mults(rng, B, N + 1, K) + [obs] if "static" in case or "moving" in case else None
                    us_d, xq_d = torch.as_tensor(us, **f64), torch.as_tensor(xs_q, **f64)
                    what = (B, K, case, sat)
                    # the restatement
                    rows = [None if x is None else (g, host(x[0][1:B + 1]), host(x[1][1:B + 1]))
                            for x, g in ((box, g_box(us, lb, ub)), (sph, g_spheres(xs_q, obs)))]
                    for r in rows:
                        if r is not None and len(sat) < B:
                            assert (r[0] > tol).any() and ((r[0] < 0).any() or r[0].size < 8), what
                    got = {}
                    for shift in (0, 1):
                        mv, mu, vb, vs, bufs = _run_step(s, B, xq_d, us_d, mu0, shift, box, sph, tol)
                        e_mv, e_mu, e_box, e_sph = al_mpc_step_restated(np.full(B, mu0), 10.0, 1e8, tol, shift, rows[0], rows[1])
                        assert np.allclose(host(mv), e_mv, rtol=RT, atol=AT), what
                        assert np.array_equal(host(mu), e_mu), what
                        for b in range(B):  # the satisfied trajectory holds mu beside the violating ones
                            assert host(mu)[b] == (mu0 if b in sat else 10 * mu0), what
                        for v, e in ((vb, e_box), (vs, e_sph)):
                            if v is not None:
                                assert np.allclose(host(v[0]), e[0], rtol=RT, atol=AT), what
                                assert np.array_equal(host(v[1]), e[1]), what
                        for pair in bufs:
                            for buf in pair or ():
                                assert (buf[0] == SENTINEL).all() and (buf[B + 1] == SENTINEL).all(), what
                        got[shift] = (mv, mu, vb, vs)
                    # the shift is data movement: bitwise the unshifted result moved by indexing
                    for v0, v1 in zip(got[0][2:], got[1][2:]):
                        if v0 is not None:
                            idx = torch.as_tensor(shifted(np.arange(v0[0].shape[1])[None])[0], device="cuda:0")
                            assert torch.equal(bits(v1[0]), bits(v0[0][:, idx])) and torch.equal(bits(v1[1]), bits(v0[1][:, idx])), what
                    assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1]))
                    # twice on equal inputs: equal bits
                    mv, mu, vb, vs, _ = _run_step(s, B, xq_d, us_d, mu0, 1, box, sph, tol)
                    for x, y in zip((mv, mu) + (vb or ()) + (vs or ()), got[1][:2] + (got[1][2] or ()) + (got[1][3] or ())):
                        assert torch.equal(bits(x), bits(y)), what


@pytest.mark.parametrize("N", [2, 40, N_LONG])
@pytest.mark.parametrize("kind", ["se3", "drone"])
def test_step_without_shift_is_update_state_when_every_problem_violates(kind, N):
    prob = _problem(kind, N)
    B, K, m, mu0, tol = 5, 3, prob.m, 0.5, 1e-2
    s = BatchedTrackingILQR(prob, B)
    for n, case in enumerate(("box", "static", "box+moving")):
        rng = np.random.default_rng(50 + n)
        lb, ub, us, xs_q, obs = _step_inputs(N, m, B, K, "moving" in case, [], 70 + n)
        box = _mults(rng, B, N, 2 * m) + [lb, ub] if "box" in case else None
        sph = _mults(rng, B, N + 1, K) + [obs] if "static" in case or "moving" in case else None
        us_d, xq_d = torch.as_tensor(us, **f64), torch.as_tensor(xs_q, **f64)
        mv, mu, vb, vs, _ = _run_step(s, B, xq_d, us_d, mu0, 0, box, sph, tol)
        assert (mv >= tol).all()
        # tolg_al_update_state on fresh copies, al_converged zero
        cb = None if box is None else (box[0][1:B + 1].clone(), box[1][1:B + 1].clone())
        cs = None if sph is None else (sph[0][1:B + 1].clone(), sph[1][1:B + 1].clone())
        if cb is not None:
            s.set_al(lb, ub, *cb)
        if cs is not None:
            s.set_al_obstacles(obs, *cs)
        mu2, mv2 = torch.full((B,), mu0, **f64), torch.zeros(B, **f64)
        conv = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        s._call("tolg_al_update_state", B, P(xq_d), P(us_d), P(mu2), 10.0, 1e8, tol, P(mv2), P(conv))
        s.set_al(None)
        s.set_al_obstacles(None)
        assert not conv.any() and np.array_equal(host(mu), host(mu2))
        assert np.allclose(host(mv), host(mv2), rtol=RT, atol=AT)
        for v, c in ((vb, cb), (vs, cs)):
            if v is not None:
                assert np.allclose(host(v[0]), host(c[0]), rtol=RT, atol=AT) and np.array_equal(host(v[1]), host(c[1])), case


# 2 -------------------------------------------------------------------------------------------------------------------
def _paths(B, T, K, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(B, T + 1, K, 4))
    a[..., 3] = rng.uniform(0.2, 0.5, (B, T + 1, K))
    return a


@pytest.mark.parametrize("T", ["1", "N-3", "N+6"])
def test_windows_are_the_moving_form_on_host_slices(T):
    B, N, K = 5, 20, 2
    T = {"1": 1, "N-3": N - 3, "N+6": N + 6}[T]
    prob, q, xi, us, _ = workloads.se3_obstacle_field(B, K, N=N)
    path = _paths(B, T, K, 3)
    path[..., :3] = 0.3 * path[..., :3] + prob.q_ref[N // 2, :3, 3]  # near the path, so that the spheres act
    t0 = (np.array([0, 3, 1, 40, 7]) % (T + 1)).astype(np.int32)
    rng = np.random.default_rng(4)
    lam = torch.as_tensor(rng.uniform(0, 1, (B, N + 1, K)), **f64)
    imu = torch.as_tensor(rng.uniform(0, 20, (B, N + 1, K)), **f64)
    s = BatchedTrackingILQR(prob, B)
    n = s.lib.tolg_obstacles_moving_bytes(C.byref(s._p), B, K) // 8
    assert n == (N + 1) * 4 * K * 8  # Bp = 8: three padded lanes
    kw = dict(mode="ms", n_iterations=5, check_every=0, **ZERO)
    for t in (0, 3, T + 2):
        s.set_al_obstacle_windows(path, t, t0=t0, lam=lam, imu=imu)
        a = s._obs_mov_buf[:n].clone()
        ra = s.fit_batch(q, xi, us, **kw)
        s._obs_mov_buf.fill_(0.0)
        sliced = path[np.arange(B)[:, None], mpc_window_index(t0, t, N, T)]
        s.set_al_obstacles(sliced, lam, imu)
        assert torch.equal(bits(a), bits(s._obs_mov_buf[:n])), t
        rb = s.fit_batch(q, xi, us, **kw)
        assert_bitwise(ra, rb, what="window gather, t = %d" % t)
    s.set_al_obstacles(None)
    r0 = s.fit_batch(q, xi, us, **kw)
    assert not torch.equal(bits(r0.us), bits(rb.us))  # the spheres act
    # t0 = None is phase 0
    s.set_al_obstacle_windows(path, 2, lam=lam, imu=imu)
    a = s._obs_mov_buf[:n].clone()
    s.set_al_obstacles(path[np.arange(B)[:, None], mpc_window_index(np.zeros(B, int), 2, N, T)], lam, imu)
    assert torch.equal(bits(a), bits(s._obs_mov_buf[:n]))
    s.set_al_obstacle_windows(None, 0)  # detaches
    assert s._obs is None
    assert_bitwise(r0, s.fit_batch(q, xi, us, **kw), what="detached")


def test_window_argument_errors():
    B, N, K, T = 3, 20, 2, 30
    prob, q, xi, us, _ = workloads.se3_obstacle_field(B, K, N=N)
    s = BatchedTrackingILQR(prob, 4)
    lib, h, st = s.lib, s._h, s._stream()
    d = torch.as_tensor(_paths(B, T, K, 1), **f64)
    lam, imu = torch.zeros(B, N + 1, K, **f64), torch.zeros(B, N + 1, K, **f64)
    buf = torch.empty(lib.tolg_obstacles_moving_bytes(C.byref(s._p), 4, 16) // 8, **f64)
    nb = C.c_size_t(buf.numel() * 8)
    t0 = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    attach = lib.tolg_set_al_obstacle_windows
    assert attach(h, B, K, P(d), 0, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == -1    # T < 1
    assert attach(h, B, K, P(d), T, P(t0), -1, P(lam), P(imu), P(buf), nb, st) == -1   # t < 0
    assert attach(h, 0, K, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, 5, K, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, B, 0, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, B, 17, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == -1
    assert attach(h, B, K, P(d), T, P(t0), 0, None, P(imu), P(buf), nb, st) == -1
    assert attach(h, B, K, P(d), T, P(t0), 0, P(lam), None, P(buf), nb, st) == -1
    assert attach(h, B, K, P(d), T, P(t0), 0, P(lam), P(imu), None, nb, st) == -1
    short = C.c_size_t(lib.tolg_obstacles_moving_bytes(C.byref(s._p), B, K) - 8)
    assert attach(h, B, K, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), short, st) == -1
    s.solve_begin(q, xi, us, n_iterations=2)
    assert attach(h, B, K, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == -1    # a solve in flight
    mu = torch.ones(B, **f64)
    s.solve_iterate(2)
    r = s.solve_end()
    # the step: nothing attached; then, attached, its own list
    step = lib.tolg_al_mpc_step
    assert step(h, B, P(r.xs_q), P(r.us), P(mu), 10.0, 1e8, 1e-2, None, 0, st) == -1
    K0 = s.gains()["K"]
    assert attach(h, B, K, P(d), T, P(t0), 0, P(lam), P(imu), P(buf), nb, st) == 0
    assert torch.equal(s.gains()["K"], K0)  # the held policy survives the attach
    adv0 = s.mpc_advance()
    assert step(h, 2, P(r.xs_q), P(r.us), P(mu), 10.0, 1e8, 1e-2, None, 0, st) == -1    # not the spheres' B
    assert step(h, 0, P(r.xs_q), P(r.us), P(mu), 10.0, 1e8, 1e-2, None, 0, st) == -1
    assert step(h, B, None, P(r.us), P(mu), 10.0, 1e8, 1e-2, None, 0, st) == -1         # spheres need the states
    assert step(h, B, P(r.xs_q), P(r.us), None, 10.0, 1e8, 1e-2, None, 0, st) == -1
    assert step(h, B, P(r.xs_q), P(r.us), P(mu), 10.0, 1e8, 1e-2, None, 2, st) == -1
    assert step(h, B, P(r.xs_q), None, P(mu), 10.0, 1e8, 1e-2, None, 1, st) == 0         # no box: no controls needed
    adv1 = s.mpc_advance()  # ... and the held policy survives the step
    for k in ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us"):
        assert same(adv0[k], adv1[k]), k
    assert attach(h, 0, 0, None, 0, None, 0, None, None, None, 0, st) == 0               # detaches
    s.set_al(np.full(6, -1.0), np.full(6, 1.0), torch.zeros(B, N, 12, **f64), torch.zeros(B, N, 12, **f64))
    assert step(h, B, None, None, P(mu), 10.0, 1e8, 1e-2, None, 0, st) == -1            # a box needs the controls
    assert step(h, B, None, P(r.us), P(mu), 10.0, 1e8, 1e-2, None, 0, st) == 0
    s.set_al(None)
    so3 = BatchedTrackingILQR(workloads.so3_tracking(2, N=20)[0], 2)
    assert so3.lib.tolg_set_al_obstacle_windows(so3._h, 2, K, P(d), T, None, 0, P(lam), P(imu), P(buf), nb, st) == -1
    for bad in (d[..., :3], d[:, :1], torch.full((B, T + 1, 17, 4), 1.0), -d):
        with pytest.raises(ValueError):
            s.set_al_obstacle_windows(bad, 0, lam=lam, imu=imu)
    with pytest.raises(ValueError):
        s.set_al_obstacle_windows(d, -1, lam=lam, imu=imu)


# 3 -------------------------------------------------------------------------------------------------------------------
LOOP = dict(first_iters=6, iters_per_step=3, first_al_iters=2, mu0=1e-2, mu_scale=10.0, mu_max=1e8, tol_constr=1e-2)


def _box_of(free):
    """A planner's box that binds without starving the loop: per input, the 90th percentile in magnitude of the inputs the
    unconstrained loop `free` (an MPCResult) applied.  (A box of +-1 on se3_mpc, whose unconstrained plans hold inputs up to 50, makes the few
    accept-always iterations of a step diverge within two steps: INTEGRATION.md 3m.)"""
    u = np.abs(host(free.us))
    lim = np.percentile(u[np.isfinite(u).all(axis=(1, 2))].reshape(-1, u.shape[-1]), 90, axis=0)
    return -lim, lim


FREE = dict(first_iters=6, iters_per_step=3, check_every=0)  # the unconstrained loop of LOOP


def _loop_from_parts(s, w, steps, warm, per_step, lb, ub):
    """mpc(lb, ub, obstacle_paths) written out from the public methods.  The reference window reaches solve_begin as host
    slices (q_ref / xi_ref: solve_begin states its own references, and tolg_set_refs on host slices packs the bits of
    tolg_set_ref_windows -- test_windows_are_set_refs_on_host_slices, tests/test_gpu_mpc.py)."""
    prob, q, xi, pq, px, t0, noise, obs, mov = w
    B, N, m, K = q.shape[0], prob.N, prob.m, mov.shape[2]
    T = pq.shape[1] - 1
    mu0 = LOOP["mu0"]
    lam, imu = torch.zeros(B, N, 2 * m, **f64), torch.full((B, N, 2 * m), mu0, **f64)
    lam_o, imu_o = torch.zeros(B, N + 1, K, **f64), torch.full((B, N + 1, K), mu0, **f64)
    mu, J = torch.full((B,), mu0, **f64), torch.zeros(B, **f64)
    out = dict(xs_q=[torch.as_tensor(q, **f64)], xs_xi=[torch.as_tensor(xi, **f64)], us=[], max_violation=[])
    x_q, x_xi, us, xs = q, xi, None, None
    s.set_al(lb, ub, lam, imu)
    try:
        for t in range(steps):
            idx = mpc_window_index(t0, t, N, T)
            refs = dict(q_ref=pq[np.arange(B)[:, None], idx], xi_ref=px[np.arange(B)[:, None], idx])
            s.set_al_obstacle_windows(mov, t, t0=t0, lam=lam_o, imu=imu_o)
            n = LOOP["first_iters"] if t == 0 else LOOP["iters_per_step"]
            rounds = LOOP["first_al_iters"] if t == 0 else per_step
            for a in range(rounds):
                if a > 0:
                    us, xs = r.us, (r.xs_q, r.xs_xi) if warm == "states" else None
                s.solve_begin(x_q, x_xi, us, mode="ms", n_iterations=n, xs_init=xs, **refs)
                s.solve_iterate(n)
                r = s.solve_end()
                mv = s.al_mpc_step(r.xs_q, r.us, mu, LOOP["mu_scale"], LOOP["mu_max"], LOOP["tol_constr"], a == rounds - 1)
            adv = s.mpc_advance(J_cl=J)
            x_q, x_xi, us = adv["x_next_q"], adv["x_next_xi"], adv["us"]
            xs = (adv["xs_q"], adv["xs_xi"]) if warm == "states" else None
            out["xs_q"].append(x_q); out["xs_xi"].append(x_xi); out["us"].append(adv["u"]); out["max_violation"].append(mv)
    finally:
        s.set_al(None)
        s.set_al_obstacles(None)
        s.clear_per_trajectory()
    return {k: torch.stack(v, dim=1) for k, v in out.items()} | dict(J=J, mu=mu)


@pytest.mark.parametrize("per_step", [1, 2])
@pytest.mark.parametrize("warm", ["states", "controls"])
def test_the_loop_is_its_parts(warm, per_step):
    B, N, steps, K = 5, 20, 4, 2
    w = workloads.se3_mpc_obstacles(B, steps, N=N, K=K, seed=21, sigma_noise=0.0)
    prob, q, xi, pq, px, t0, noise, obs, mov = w
    s = BatchedTrackingILQR(prob, B)
    lb, ub = _box_of(s.mpc(q, xi, pq, px, steps, t0=t0, warm=warm, **FREE))
    r = s.mpc(q, xi, pq, px, steps, t0=t0, warm=warm, check_every=0, lb=lb, ub=ub, obstacle_paths=mov,
              al_iters_per_step=per_step, **LOOP)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "clearance"):
        assert np.isfinite(host(getattr(r, k))).all(), k
    assert (host(r.status) == _capi.ST_OK).all()
    e = _loop_from_parts(BatchedTrackingILQR(prob, B), w, steps, warm, per_step, lb, ub)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu"):
        assert torch.equal(bits(getattr(r, k)), bits(e[k])), k
    assert (r.mu > LOOP["mu0"]).any() and r.clearance.shape == (B, steps + 1)
    # clearance: the realised states against the spheres of their world knots
    for b in range(B):
        for k in range(steps + 1):
            c = mov[b, min(t0[b] + k, mov.shape[1] - 1)]
            d = (np.linalg.norm(host(r.xs_q)[b, k, :3, 3] - c[:, :3], axis=1) - c[:, 3]).min()
            assert abs(host(r.clearance)[b, k] - d) < 1e-12


def test_batch_independence():
    B, N, steps, K = 13, 20, 3, 2
    prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, steps, N=N, K=K, seed=22)
    s = BatchedTrackingILQR(prob, B)
    lb, ub = _box_of(s.mpc(q, xi, pq, px, steps, t0=t0, noise=noise, **FREE))
    kw = dict(warm="states", check_every=0, lb=lb, ub=ub, **LOOP)
    r = s.mpc(q, xi, pq, px, steps, t0=t0, noise=noise, obstacle_paths=mov, **kw)
    assert np.isfinite(host(r.us)).all() and (host(r.status) == _capi.ST_OK).all()
    rows = slice(4, 8)
    r4 = BatchedTrackingILQR(prob, 4).mpc(q[rows], xi[rows], pq[rows], px[rows], steps, t0=t0[rows], noise=noise[rows],
                                         obstacle_paths=mov[rows], **kw)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "clearance", "iters", "status"):
        assert torch.equal(bits(getattr(r, k)[rows]), bits(getattr(r4, k))), k


def test_device_paths_stay_on_the_device_and_shared_spheres_broadcast():
    """obstacle_paths as a tensor on the solver's device is checked there and used as it is -- no copy through the host -- and
    gives the bits of the same paths from the host; a bad value in it is still refused.  obstacles [K, 4] is [B, K, 4] with
    every trajectory's spheres the same."""
    B, N, steps, K = 5, 20, 3, 2
    prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, steps, N=N, K=K, seed=26)
    s = BatchedTrackingILQR(prob, B)
    kw = dict(t0=t0, noise=noise, warm="states", check_every=0, **LOOP)
    r = s.mpc(q, xi, pq, px, steps, obstacle_paths=mov, **kw)
    d = torch.as_tensor(mov, **f64)
    seen = []
    rd = s.mpc(q, xi, pq, px, steps, obstacle_paths=d, on_step=lambda t, out: seen.append(s._obs[0].data_ptr()), **kw)
    assert seen == [d.data_ptr()] * steps  # the handle gathers from the caller's tensor itself
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "clearance"):
        assert torch.equal(bits(getattr(r, k)), bits(getattr(rd, k))), k
    assert s._check_obstacle_paths(B, d)[1] is d and s._check_obstacle_paths(None, d)[0] == B
    for i, v in ((0, float("nan")), (0, float("inf")), (3, 0.0), (3, -1.0)):
        bad = d.clone()
        bad[2, 1, 1, i] = v
        with pytest.raises(ValueError):
            s.mpc(q, xi, pq, px, steps, obstacle_paths=bad, **kw)
        with pytest.raises(ValueError):
            s.set_al_obstacle_windows(bad, 0)
        assert s._al is None and s._obs is None
    shared = obs[0]
    ra = s.mpc(q, xi, pq, px, steps, obstacles=shared, **kw)
    rb = s.mpc(q, xi, pq, px, steps, obstacles=np.ascontiguousarray(np.broadcast_to(shared, (B, K, 4))), **kw)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "clearance"):
        assert torch.equal(bits(getattr(ra, k)), bits(getattr(rb, k))), k
    assert ra.clearance.shape == (B, steps + 1) and (ra.mu > LOOP["mu0"]).any()


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["static", "paths", "box", "box+paths"])
def test_zero_penalty_is_the_unconstrained_loop(form):
    """With mu0 = 0 every multiplier and every I_mu stays zero, and zero terms change no bit of a solve: for the spheres
    test_zero_multipliers_change_nothing shows it (tests/test_gpu_obstacles.py); for the box, fit_batch behind a set_al with zero
    lambda and I_mu was compared with the plain fit_batch on the parent commit (se3, B = 5, N = 20, 6 iterations, with and without
    tolerances) and gave equal bits in us and xs_q -- so the box is included here."""
    B, N, steps, K = 5, 20, 4, 2
    prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, steps, N=N, K=K, seed=23)
    kw = dict(t0=t0, noise=noise, first_iters=6, iters_per_step=3, warm="states", check_every=0)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.mpc(q, xi, pq, px, steps, **kw)
    con = dict(obstacles=obs) if form == "static" else dict(obstacle_paths=mov) if "paths" in form else {}
    if "box" in form:
        con.update(zip(("lb", "ub"), _box_of(r0)))
    r1 = s.mpc(q, xi, pq, px, steps, mu0=0.0, first_al_iters=1, al_iters_per_step=1, **con, **kw)
    for k in ("xs_q", "xs_xi", "us", "J", "iters", "status"):
        assert torch.equal(bits(getattr(r0, k)), bits(getattr(r1, k))), k
    assert (r1.mu == 0).all() and r1.max_violation.shape == (B, steps) and r0.max_violation is None and r0.clearance is None


# 5 -------------------------------------------------------------------------------------------------------------------
def _does_something():
    B, N, steps, K = 4, 40, 30, 1
    return workloads.se3_mpc_obstacles(B, steps, N=N, K=K, seed=24, sigma_noise=0.0), steps


def _clearance(xs_q, obs):
    t = host(xs_q)[:, :, None, :3, 3]
    return (np.linalg.norm(t - obs[:, None, :, :3], axis=-1) - obs[:, None, :, 3]).min(axis=(1, 2))


def test_spheres_in_the_planner_reduce_the_penetration():
    (prob, q, xi, pq, px, t0, noise, obs, mov), steps = _does_something()
    kw = dict(t0=t0, first_iters=30, iters_per_step=5, warm="states", check_every=0)
    s = BatchedTrackingILQR(prob, q.shape[0])
    free = _clearance(s.mpc(q, xi, pq, px, steps, **kw).xs_q, obs)
    print("unconstrained clearance", free)
    assert (free < 0).all()  # a condition on the inputs: the unconstrained loop flies through every sphere
    r = s.mpc(q, xi, pq, px, steps, obstacles=obs, **kw)
    con = host(r.clearance).min(axis=1)
    print("constrained clearance", con, "max_violation first / last", host(r.max_violation)[:, 0], host(r.max_violation)[:, -1])
    assert np.allclose(con, _clearance(r.xs_q, obs), rtol=0, atol=1e-12)
    assert (np.minimum(con, 0.0) > free).all()  # the worst penetration is strictly smaller for every trajectory
    assert (host(r.max_violation)[:, -1] < host(r.max_violation)[:, 0]).all()


def test_a_box_in_the_planner_reduces_the_saturation():
    (prob, q, xi, pq, px, t0, noise, obs, mov), steps = _does_something()
    kw = dict(t0=t0, first_iters=30, iters_per_step=5, warm="states", check_every=0)
    s = BatchedTrackingILQR(prob, q.shape[0])
    u = np.abs(host(s.mpc(q, xi, pq, px, steps, **kw).us))
    lim = np.percentile(u.reshape(-1, prob.m), 90, axis=0)  # per input: a tenth of the unconstrained loop's inputs exceed it
    clip = s.mpc(q, xi, pq, px, steps, u_lb=-lim, u_ub=lim, **kw)
    plan = s.mpc(q, xi, pq, px, steps, u_lb=-lim, u_ub=lim, lb=-lim, ub=lim, **kw)
    n_clip, n_plan = int(clip.n_sat.sum()), int(plan.n_sat.sum())
    print("n_sat: the plant clips alone", n_clip, "with the planner's box", n_plan)
    assert n_clip > 0 and n_plan < n_clip


# 6 -------------------------------------------------------------------------------------------------------------------
def test_the_handle_is_left_clean_and_the_argument_errors():
    B, N, steps, K = 5, 20, 3, 2
    prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, steps, N=N, K=K, seed=25)
    fit = dict(mode="ms", n_iterations=5, check_every=0, **ZERO)
    fresh = BatchedTrackingILQR(prob, B).fit_batch(q, xi, None, **fit)
    s = BatchedTrackingILQR(prob, B)
    kw = dict(t0=t0, first_iters=4, iters_per_step=2, check_every=0)
    lb, ub = _box_of(s.mpc(q, xi, pq, px, steps, **kw))
    s.mpc(q, xi, pq, px, steps, lb=lb, ub=ub, obstacle_paths=mov, **kw)
    assert s._al is None and s._obs is None
    assert_bitwise(fresh, s.fit_batch(q, xi, None, **fit), what="behind mpc")

    def stop(t, out):
        if t == 1:
            raise KeyError("stop")

    with pytest.raises(KeyError):
        s.mpc(q, xi, pq, px, steps, lb=lb, ub=ub, obstacles=obs, on_step=stop, **kw)
    assert s._al is None and s._obs is None
    assert_bitwise(fresh, s.fit_batch(q, xi, None, **fit), what="behind an mpc that raised")
    for bad in (dict(lb=lb, ub=ub, mode="ss", warm="controls"), dict(obstacles=obs, mode="ss", warm="controls"),
                dict(obstacles=obs, obstacle_paths=mov), dict(lb=lb), dict(obstacles=np.ones((B, 17, 4))),
                dict(obstacle_paths=np.ones((B, 9, 17, 4))), dict(obstacle_paths=mov[:4]), dict(obstacles=obs[:4]),
                dict(obstacle_paths=mov[..., :3]), dict(lb=lb, ub=ub, first_al_iters=0), dict(lb=lb[:3], ub=ub[:3])):
        with pytest.raises(ValueError):
            s.mpc(q, xi, pq, px, steps, **bad, **kw)
        assert s._al is None and s._obs is None
    # a constraint the caller attached is still refused
    s.set_al(lb, ub, torch.zeros(B, N, 12, **f64), torch.zeros(B, N, 12, **f64))
    with pytest.raises(ValueError, match="augmented-Lagrangian"):
        s.mpc(q, xi, pq, px, steps, **kw)
    s.set_al(None)
    # the SO3 family: the box, not the spheres
    p3, q3, x3, _ = workloads.so3_tracking(2, N=N)
    path_q = np.broadcast_to(p3.q_ref, (2,) + p3.q_ref.shape)
    path_x = np.broadcast_to(p3.xi_ref, (2,) + p3.xi_ref.shape)
    s3 = BatchedTrackingILQR(p3, 2)
    for con in (dict(obstacles=np.ones((1, 4))), dict(obstacle_paths=np.ones((2, 9, 1, 4)))):
        with pytest.raises(ValueError, match="translation"):
            s3.mpc(q3, x3, path_q, path_x, 2, **con)
    b3 = np.r_[np.full(3, 0.5), np.full(3, 1.0)]
    r3 = s3.mpc(q3, x3, path_q, path_x, 2, first_iters=4, iters_per_step=2, lb=-b3, ub=b3)
    assert np.isfinite(host(r3.us)).all() and r3.clearance is None and r3.max_violation.shape == (2, 2)


# 7 -------------------------------------------------------------------------------------------------------------------
def test_full_size():
    """The first three steps of a loop whose spheres lie 10 .. 30 knots ahead, inside every step's horizon"""
    B, N, steps, K = 4096, 200, 3, 4
    prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, 40, N=N, K=K)
    noise = noise[:, :steps]
    kw = dict(first_iters=5, iters_per_step=5, warm="states", check_every=0)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.mpc(q, xi, pq, px, steps, t0=t0, noise=noise, **kw)
    lb, ub = _box_of(r0)
    con = dict(lb=lb, ub=ub, **{k: LOOP[k] for k in ("mu0", "mu_scale", "mu_max", "tol_constr")})
    r = s.mpc(q, xi, pq, px, steps, t0=t0, noise=noise, obstacle_paths=mov, **con, **kw)
    ok = (host(r0.status) == _capi.ST_OK).all(axis=1)
    assert ok.sum() > B // 2
    assert (host(r.status)[ok] == _capi.ST_OK).all()
    for f in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "clearance"):
        assert np.isfinite(host(getattr(r, f))[ok]).all(), f
    rows = slice(64 * 17 + 8, 64 * 17 + 12)
    r4 = BatchedTrackingILQR(prob, 4).mpc(q[rows], xi[rows], pq[rows], px[rows], steps, t0=t0[rows], noise=noise[rows],
                                         obstacle_paths=mov[rows], **con, **kw)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "clearance", "iters", "status"):
        assert torch.equal(bits(getattr(r, k)[rows]), bits(getattr(r4, k))), k
