"""Attitude constraints in receding-horizon MPC and fleet planning: the pose slots (tilt cones, view cones) as the third row set
of the step (tolg_al_mpc_step_pose), their window form, mpc(pose_constraints= / pose_paths=) and plan_fleet(pose_constraints=).

1.  tolg_al_mpc_step_pose against the three-set restatement of tests/pose_mpc.py: every shape at which the kernel takes another path,
    every combination of row sets, the in-place shift bitwise, sentinels, repeatability;
2.  ... and against tolg_al_update_state where both apply;
3.  the box and sphere rows do not see the family;
4.  tolg_set_al_pose_constraint_windows: the packed bits of the per-knot form on host-sliced windows, argument errors;
5.  mpc(pose_paths=) is its parts, bitwise;
6.  batch independence;
7.  with mu0 = 0 the constrained loop gives the bits of the unconstrained one;
8.  it does something: a larger margin than the unconstrained loop's in every trajectory;
9.  plan_fleet(pose_constraints=): every round is al_fit_batch on its rows;
10. the handle's state behind mpc(), and the argument errors.

Tolerances are those of tests/test_gpu_mpc_constrained.py: maxviol and lambda rtol 1e-12 with the 1e-15 floor, mu and I_mu exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, workloads
from trajectory_optimization_matrix_lie_groups_amd.solver import mpc_window_index, pose_margin
from tests import pose_kinds as pk
from tests import pose_mpc as pm
from tests.mpc_al import shifted
from tests.support import ZERO, assert_bitwise, bits, host
from tests.test_gpu_mpc_constrained import AT, FREE, LOOP, RT, SENTINEL, _box_of, _problem

pytestmark = pytest.mark.gpu
f64 = dict(dtype=torch.float64, device="cuda:0")
P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
SETS = ("box", "sph", "pose")
KS = 3  # the spheres beside the pose slots


def _on_device(c, B):
    """A step_case's controls and poses on the device, its multipliers as views between two sentinel trajectories"""
    d = dict(us=torch.as_tensor(c["us"], **f64), xs_q=torch.as_tensor(c["xs_q"], **f64))
    for k in SETS:
        d[k] = None
        if c[k] is not None:
            d[k] = []
            for a in c[k]:
                buf = torch.full((B + 2,) + a.shape[1:], SENTINEL, **f64)
                buf[1:B + 1] = torch.as_tensor(a, **f64)
                d[k].append(buf)
    return d


def _run_step(s, B, c, d, mu0, shift, tol=1e-2, pose=True):
    """One al_mpc_step() (tolg_al_mpc_step_pose with the pose slots attached, tolg_al_mpc_step without) on fresh copies of the multiplier buffers of whatever the case attaches (pose=False: without the pose
    slots).  Returns (maxviol, mu, {set: (lam, imu) views or None}, the buffers)."""
    bufs = {k: None if d[k] is None or (k == "pose" and not pose) else [x.clone() for x in d[k]] for k in SETS}
    v = {k: None if x is None else (x[0][1:B + 1], x[1][1:B + 1]) for k, x in bufs.items()}
    try:
        if v["box"] is not None:
            s.set_al(c["lb"], c["ub"], *v["box"])
        if v["sph"] is not None:
            s.set_al_obstacles(c["obs"], *v["sph"])
        if v["pose"] is not None:
            s.set_al_pose_constraints(c["slots"], c["kinds"], *v["pose"])
        mu = torch.full((B,), mu0, **f64)
        mv = s.al_mpc_step(d["xs_q"], d["us"] if v["box"] is not None else None, mu, 10.0, 1e8, tol, shift)
    finally:
        s.set_al(None)
        s.set_al_obstacles(None)
        s.set_al_pose_constraints(None)
    return mv, mu, v, bufs


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 7, 40, pm.N_LONG])
@pytest.mark.parametrize("kind", ["se3", "drone"])
def test_step_against_the_restatement(kind, N):
    prob = _problem(kind, N)
    m, mu0, tol = prob.m, 0.5, 1e-2
    solvers = {}
    for B, Kp, case, sat, seed in pm.step_grid(N):
        s = solvers.setdefault(B, BatchedTrackingILQR(prob, B))
        what = (B, Kp, case, sat)
        c = pm.step_case(N, m, B, KS, Kp, case, sat, seed)
        rows = pm.step_rows(c)
        # I_mu' is compared exactly: no row may sit at a branch point of the rule, where the kernel's rounding of a row (the view
        # row holds a square root) could choose otherwise
        assert pm.clear_of_branch_points(rows) > pm.CLEAR, what
        # ... and lambda' at the floor of its tolerance: no row's rounding, times its I_mu, may exceed what the comparison allows
        assert pm.lambda_error_bound(c, rows) < 1.0, what
        if len(sat) < B:  # every slot acts on both sides
            g = rows[2][0]
            assert (g > tol).any() and (g < 0).any(), what
        d = _on_device(c, B)
        got = {}
        for shift in (0, 1):
            mv, mu, v, bufs = _run_step(s, B, c, d, mu0, shift, tol)
            e = pm.al_mpc_step_restated3(np.full(B, mu0), 10.0, 1e8, tol, shift, *rows)
            assert np.allclose(host(mv), e[0], rtol=RT, atol=AT), what
            assert np.array_equal(host(mu), e[1]), what
            for b in range(B):  # the satisfied trajectory holds mu beside the violating ones
                assert host(mu)[b] == (mu0 if b in sat else 10 * mu0), what
            for k, want in zip(SETS, e[2:]):
                assert (v[k] is None) == (want is None), what
                if want is not None:
                    assert np.allclose(host(v[k][0]), want[0], rtol=RT, atol=AT), (what, k)
                    assert np.array_equal(host(v[k][1]), want[1]), (what, k)
                    for buf in bufs[k]:
                        assert (buf[0] == SENTINEL).all() and (buf[B + 1] == SENTINEL).all(), (what, k)
            got[shift] = (mv, mu, v)
        # the shift is data movement: bitwise the unshifted result moved by indexing
        for k in SETS:
            v0, v1 = got[0][2][k], got[1][2][k]
            if v0 is not None:
                idx = torch.as_tensor(shifted(np.arange(v0[0].shape[1])[None])[0], device="cuda:0")
                assert torch.equal(bits(v1[0]), bits(v0[0][:, idx])) and torch.equal(bits(v1[1]), bits(v0[1][:, idx])), (what, k)
        assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1])), what
        # twice on equal inputs: equal bits
        mv, mu, v, _ = _run_step(s, B, c, d, mu0, 1, tol)
        assert torch.equal(bits(mv), bits(got[1][0])) and torch.equal(bits(mu), bits(got[1][1])), what
        for k in SETS:
            for x, y in zip(v[k] or (), got[1][2][k] or ()):
                assert torch.equal(bits(x), bits(y)), (what, k)


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 40, pm.N_LONG])
@pytest.mark.parametrize("kind", ["se3", "drone"])
def test_step_without_shift_is_update_state_when_every_problem_violates(kind, N):
    prob = _problem(kind, N)
    B, Kp, m, mu0, tol = 5, 3, prob.m, 0.5, 1e-2
    s = BatchedTrackingILQR(prob, B)
    for n, case in enumerate(("pose", "box+pose_knot", "static+pose")):
        c = pm.step_case(N, m, B, KS, Kp, case, [], 300 + 10 * N + n)
        d = _on_device(c, B)
        mv, mu, v, _ = _run_step(s, B, c, d, mu0, 0, tol)
        assert (mv >= tol).all()
        # tolg_al_update_state on fresh copies, al_converged zero
        cp = {k: None if d[k] is None else (d[k][0][1:B + 1].clone(), d[k][1][1:B + 1].clone()) for k in SETS}
        if cp["box"] is not None:
            s.set_al(c["lb"], c["ub"], *cp["box"])
        if cp["sph"] is not None:
            s.set_al_obstacles(c["obs"], *cp["sph"])
        s.set_al_pose_constraints(c["slots"], c["kinds"], *cp["pose"])
        mu2, mv2 = torch.full((B,), mu0, **f64), torch.zeros(B, **f64)
        conv = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        s._call("tolg_al_update_state", B, P(d["xs_q"]), P(d["us"]), P(mu2), 10.0, 1e8, tol, P(mv2), P(conv))
        s.set_al(None)
        s.set_al_obstacles(None)
        s.set_al_pose_constraints(None)
        assert not conv.any() and np.array_equal(host(mu), host(mu2))
        assert np.allclose(host(mv), host(mv2), rtol=RT, atol=AT)
        for k in SETS:
            if cp[k] is not None:
                assert np.allclose(host(v[k][0]), host(cp[k][0]), rtol=RT, atol=AT), (case, k)
                assert np.array_equal(host(v[k][1]), host(cp[k][1])), (case, k)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, pm.N_LONG])
def test_box_and_sphere_rows_are_unaffected_by_the_family(N):
    """Every pose slot is satisfied by a wide margin (every trajectory upright under the `sat` slots of step_case, rows below
    -0.4), so mv and mu_new are those of the box and the spheres alone: what the step leaves in their multipliers is, bit for
    bit, what it leaves without the family."""
    prob = _problem("se3", N)
    B, Kp, mu0 = 5, 3, 0.5
    s = BatchedTrackingILQR(prob, B)
    c = pm.step_case(N, prob.m, B, KS, Kp, "box+moving+pose_knot", [], 41)
    far = pm.step_case(N, prob.m, B, KS, Kp, "box+moving+pose_knot", list(range(B)), 41)
    c["xs_q"][..., :3, :3] = np.eye(3)  # the spheres read the positions alone
    c["slots"] = far["slots"] - np.r_[1000.0, 1000.0, 1000.0, 0.0] * (np.array(c["kinds"]) == pk.VIEW)[:, None]
    assert pk.g_rows(c["xs_q"], c["slots"], c["kinds"]).max() < -0.4
    d = _on_device(c, B)
    for shift in (0, 1):
        mv1, mu1, v1, _ = _run_step(s, B, c, d, mu0, shift)
        mv0, mu0_, v0, _ = _run_step(s, B, c, d, mu0, shift, pose=False)
        assert (mv1 >= 1e-2).all() and v0["pose"] is None
        assert torch.equal(bits(mv1), bits(mv0)) and torch.equal(bits(mu1), bits(mu0_))
        for k in ("box", "sph"):
            assert torch.equal(bits(v1[k][0]), bits(v0[k][0])) and torch.equal(bits(v1[k][1]), bits(v0[k][1])), k
        assert not torch.equal(bits(v1["pose"][0]), bits(d["pose"][0][1:B + 1]))  # the pose multipliers did relax


# 4 -------------------------------------------------------------------------------------------------------------------
WKINDS = (pk.TILT, pk.VIEW)


def _pose_paths(prob, B, T, seed):
    """World-time slots [B, T+1, 2, 4] about the reference's middle: a tilt cone whose axis and cosine change with the knot, a view
    cone on a target that wanders 2 .. 4 away"""
    rng = np.random.default_rng(seed)
    a = np.empty((B, T + 1, 2, 4))
    n = rng.normal(size=(B, T + 1, 3))
    a[:, :, 0, :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    a[:, :, 0, 3] = rng.uniform(-0.5, 0.5, (B, T + 1))
    d = rng.normal(size=(B, T + 1, 3))
    a[:, :, 1, :3] = prob.q_ref[prob.N // 2, :3, 3] + rng.uniform(2.0, 4.0, (B, T + 1, 1)) * d / np.linalg.norm(d, axis=-1, keepdims=True)
    a[:, :, 1, 3] = rng.uniform(0.2, 0.8, (B, T + 1))
    return a


@pytest.mark.parametrize("T", ["1", "N-3", "N+6"])
def test_windows_are_the_per_knot_form_on_host_slices(T):
    B, N, K = 5, 20, 2
    T = {"1": 1, "N-3": N - 3, "N+6": N + 6}[T]
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    path = _pose_paths(prob, B, T, 3)
    t0 = np.array([0, 3, 1, T + 5, 7], dtype=np.int32)  # phases beyond the path's end hold its last knot
    rng = np.random.default_rng(4)
    lam = torch.as_tensor(rng.uniform(0, 1, (B, N + 1, K)), **f64)
    imu = torch.as_tensor(rng.uniform(0, 20, (B, N + 1, K)), **f64)
    s = BatchedTrackingILQR(prob, B)
    n = s.lib.tolg_pose_constraints_bytes(C.byref(s._p), B, K, 1) // 8
    assert n == (N + 1) * 4 * K * 8  # Bp = 8: three padded lanes
    kw = dict(mode="ms", n_iterations=5, check_every=0, **ZERO)
    r0 = s.fit_batch(q, xi, us, **kw)  # never attached
    for t in (0, 3, T + 2):
        s.set_al_pose_constraint_windows(path, t, t0=t0, kinds=WKINDS, lam=lam, imu=imu)
        assert s._pose[3] == WKINDS
        a = s._pose_knot_buf[:n].clone()
        ra = s.fit_batch(q, xi, us, **kw)
        s._pose_knot_buf.fill_(0.0)
        sliced = path[np.arange(B)[:, None], mpc_window_index(t0, t, N, T)]
        s.set_al_pose_constraints(sliced, WKINDS, lam, imu)
        assert torch.equal(bits(a), bits(s._pose_knot_buf[:n])), t
        rb = s.fit_batch(q, xi, us, **kw)
        assert_bitwise(ra, rb, what="window gather, t = %d" % t)
    assert not torch.equal(bits(r0.us), bits(rb.us))  # the slots act
    # t0 = None is phase 0
    s.set_al_pose_constraint_windows(path, 2, kinds=WKINDS, lam=lam, imu=imu)
    a = s._pose_knot_buf[:n].clone()
    s.set_al_pose_constraints(path[np.arange(B)[:, None], mpc_window_index(np.zeros(B, int), 2, N, T)], WKINDS, lam, imu)
    assert torch.equal(bits(a), bits(s._pose_knot_buf[:n]))
    s.set_al_pose_constraint_windows(None, 0)  # detaches
    assert s._pose is None
    assert_bitwise(r0, s.fit_batch(q, xi, us, **kw), what="detached")


def test_window_argument_errors():
    B, N, K, T = 3, 20, 2, 30
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, 4)
    lib, h = s.lib, s._h
    path = _pose_paths(prob, B, T, 1)
    d = torch.as_tensor(path, **f64)
    lam, imu = torch.zeros(B, N + 1, K, **f64), torch.full((B, N + 1, K), 5.0, **f64)
    buf = torch.zeros(lib.tolg_pose_constraints_bytes(C.byref(s._p), 4, _capi.MAX_POSE_CONSTRAINTS, 1) // 8, **f64)
    full = buf.numel() * 8
    t0 = torch.zeros(B, dtype=torch.int32, device="cuda:0")

    def attach(B=B, K=K, kinds=WKINDS, d=d, T=T, t0=t0, t=0, lam=lam, imu=imu, buf=buf, nbytes=full, on=s):
        kd = None if kinds is None else (C.c_int32 * len(kinds))(*kinds)
        with torch.cuda.device(on.device):
            return on.lib.tolg_set_al_pose_constraint_windows(on._h, B, K, kd, P(d), T, P(t0), t, P(lam), P(imu), P(buf),
                                                              C.c_size_t(nbytes), on._stream())

    def attached():
        mu, mv, cv = torch.ones(B, **f64), torch.zeros(B, **f64), torch.zeros(B, dtype=torch.int32, device="cuda:0")
        with torch.cuda.device(s.device):
            return lib.tolg_al_update_state(h, B, P(torch.as_tensor(np.tile(np.eye(4), (B, N + 1, 1, 1)), **f64)), None, P(mu),
                                            1.0, 1e8, 1e30, P(mv), P(cv), s._stream()) == 0

    def refused():
        short = lib.tolg_pose_constraints_bytes(C.byref(s._p), B, K, 1) - 8
        assert attach(T=0) == -1 and attach(t=-1) == -1                      # T < 1, t < 0
        assert attach(nbytes=short) == -1 and attach(buf=None) == -1         # short packed_bytes
        assert attach(kinds=(0, 2)) == -1 and attach(kinds=(-1, 1)) == -1 and attach(kinds=None) == -1   # a kind outside 0..1
        assert attach(B=0) == -1 and attach(B=5) == -1 and attach(K=0) == -1
        assert attach(K=_capi.MAX_POSE_CONSTRAINTS + 1, kinds=(0,) * (_capi.MAX_POSE_CONSTRAINTS + 1)) == -1
        assert attach(lam=None) == -1 and attach(imu=None) == -1

    refused()
    assert not attached() and not buf.any()              # a refused call attaches nothing and packs nothing
    assert attach(t=4) == 0 and attached()
    kw = dict(mode="ms", n_iterations=5, check_every=0, **ZERO)
    before, ra = buf.clone(), s.fit_batch(q, xi, us, **kw)
    refused()                                             # ... and changes nothing of what is attached
    s.solve_begin(q, xi, us, n_iterations=2)
    assert attach() == -1                                 # a solve in flight
    s.solve_iterate(2)
    s.solve_end()
    assert attached() and torch.equal(bits(before), bits(buf))
    assert_bitwise(ra, s.fit_batch(q, xi, us, **kw), what="behind refused calls")
    # the step's own list with the family attached: its B, the poses
    mu = torch.ones(B, **f64)
    xq = torch.as_tensor(np.tile(np.eye(4), (B, N + 1, 1, 1)), **f64)
    with torch.cuda.device(s.device):
        step = lambda B_, x: lib.tolg_al_mpc_step_pose(h, B_, P(x), None, P(mu), 10.0, 1e8, 1e-2, None, 0, s._stream())  # noqa: E731
        assert step(2, xq) == -1 and step(B, None) == -1
        assert lib.tolg_al_mpc_step(h, B, P(xq), None, P(mu), 10.0, 1e8, 1e-2, None, 0, s._stream()) == -1   # keeps refusing the family
        assert step(B, xq) == 0
    assert attach(d=None, B=0, K=0, kinds=None, lam=None, imu=None, buf=None, nbytes=0, T=0) == 0 and not attached()   # detaches
    so3 = BatchedTrackingILQR(workloads.so3_tracking(2, N=N)[0], 2)
    assert attach(B=2, t0=None, lam=lam[:2].contiguous(), imu=imu[:2].contiguous(), on=so3) == -1   # the SO3 family
    with pytest.raises(ValueError):
        so3.set_al_pose_constraint_windows(path[:2], 0, kinds=WKINDS)
    flat = path.copy()
    flat[1, 2, 0, :3] *= 1.1   # a tilt axis that is not unit, at one knot of the path
    wide = path.copy()
    wide[0, T, 1, 3] = 1.0     # a cosine of 1, at the last knot
    for bad in (path[..., :3], path[:, :1], np.ones((B, T + 1, 9, 4)), flat, wide):
        with pytest.raises(ValueError):
            s.set_al_pose_constraint_windows(bad, 0, kinds=WKINDS if bad.shape[2] == 2 else (0,) * 9, lam=lam, imu=imu)
    for t, kinds in ((-1, WKINDS), (0, None), (0, (0, 2)), (0, WKINDS[:1])):
        with pytest.raises(ValueError):
            s.set_al_pose_constraint_windows(path, t, kinds=kinds, lam=lam, imu=imu)
    assert s._pose is None


# 5 -------------------------------------------------------------------------------------------------------------------
def _margin(xs_q, paths, t0, kinds):
    """min_k pose_margin of realised states [B, S+1, 4, 4] under the slots of their world knots t0[b] + s, on the host"""
    B, S1 = xs_q.shape[:2]
    world = np.clip(np.asarray(t0)[:, None] + np.arange(S1)[None], 0, paths.shape[1] - 1)
    return pose_margin(host(xs_q), paths[np.arange(B)[:, None], world], kinds).min(axis=-1)


def _loop_from_parts(s, w, steps, warm, per_step):
    """mpc(pose_paths=) written out from the public methods.  The reference window reaches solve_begin as host slices, as in
    tests/test_gpu_mpc_constrained.py: solve_begin states its own references, and tolg_set_refs on host slices packs the bits of
    tolg_set_ref_windows (test_windows_are_set_refs_on_host_slices, tests/test_gpu_mpc.py)."""
    prob, q, xi, pq, px, t0, noise, paths, kinds = w
    B, N, K = q.shape[0], prob.N, paths.shape[2]
    T = pq.shape[1] - 1
    mu0 = LOOP["mu0"]
    lam, imu = torch.zeros(B, N + 1, K, **f64), torch.full((B, N + 1, K), mu0, **f64)
    mu, J = torch.full((B,), mu0, **f64), torch.zeros(B, **f64)
    out = dict(xs_q=[torch.as_tensor(q, **f64)], xs_xi=[torch.as_tensor(xi, **f64)], us=[], max_violation=[])
    x_q, x_xi, us, xs = q, xi, None, None
    try:
        for t in range(steps):
            idx = mpc_window_index(t0, t, N, T)
            refs = dict(q_ref=pq[np.arange(B)[:, None], idx], xi_ref=px[np.arange(B)[:, None], idx])
            s.set_al_pose_constraint_windows(paths, t, t0=t0, kinds=kinds, lam=lam, imu=imu)
            n = LOOP["first_iters"] if t == 0 else LOOP["iters_per_step"]
            rounds = LOOP["first_al_iters"] if t == 0 else per_step
            for a in range(rounds):
                if a > 0:
                    us, xs = r.us, (r.xs_q, r.xs_xi) if warm == "states" else None
                s.solve_begin(x_q, x_xi, us, mode="ms", n_iterations=n, xs_init=xs, **refs)
                s.solve_iterate(n)
                r = s.solve_end()
                mv = s.al_mpc_step(r.xs_q, None, mu, LOOP["mu_scale"], LOOP["mu_max"], LOOP["tol_constr"], a == rounds - 1)
            adv = s.mpc_advance(J_cl=J)
            x_q, x_xi, us = adv["x_next_q"], adv["x_next_xi"], adv["us"]
            xs = (adv["xs_q"], adv["xs_xi"]) if warm == "states" else None
            out["xs_q"].append(x_q); out["xs_xi"].append(x_xi); out["us"].append(adv["u"]); out["max_violation"].append(mv)
    finally:
        s.set_al_pose_constraint_windows(None, 0)
        s.clear_per_trajectory()
    return {k: torch.stack(v, dim=1) for k, v in out.items()} | dict(J=J, mu=mu)


@pytest.mark.parametrize("per_step", [1, 2])
@pytest.mark.parametrize("warm", ["states", "controls"])
def test_the_loop_is_its_parts(warm, per_step):
    B, N, steps = 4, 20, 4
    w = workloads.se3_mpc_inspection(B, 8, N=N, seed=21, sigma_noise=0.0)
    prob, q, xi, pq, px, t0, noise, paths, kinds = w
    s = BatchedTrackingILQR(prob, B)
    r = s.mpc(q, xi, pq, px, steps, t0=t0, warm=warm, check_every=0, pose_paths=paths, pose_kinds=kinds,
              al_iters_per_step=per_step, **LOOP)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "pose_margin"):
        assert np.isfinite(host(getattr(r, k))).all(), k
    assert (host(r.status) == _capi.ST_OK).all() and r.clearance is None
    e = _loop_from_parts(BatchedTrackingILQR(prob, B), w, steps, warm, per_step)
    for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu"):
        assert torch.equal(bits(getattr(r, k)), bits(e[k])), k
    assert (r.mu > LOOP["mu0"]).any() and r.pose_margin.shape == (B, steps + 1)
    # pose_margin: the realised states against the slots of their world knots, pose_margin()'s own arithmetic
    assert np.allclose(host(r.pose_margin), _margin(r.xs_q, paths, t0, kinds), rtol=0, atol=1e-12)


# 6 -------------------------------------------------------------------------------------------------------------------
def test_batch_independence():
    B, N, steps = 7, 20, 3
    prob, q, xi, pq, px, t0, noise, paths, kinds = workloads.se3_mpc_inspection(B, 8, N=N, seed=22)
    noise = noise[:, :steps]
    s = BatchedTrackingILQR(prob, B)
    lb, ub = _box_of(s.mpc(q, xi, pq, px, steps, t0=t0, noise=noise, **FREE))
    kw = dict(warm="states", check_every=0, lb=lb, ub=ub, pose_kinds=kinds, **LOOP)
    r = s.mpc(q, xi, pq, px, steps, t0=t0, noise=noise, pose_paths=paths, **kw)
    assert np.isfinite(host(r.us)).all() and (host(r.status) == _capi.ST_OK).all()
    for rows in (slice(3, 4), slice(5, 7)):  # a trajectory alone, and the last two
        n = rows.stop - rows.start
        ra = BatchedTrackingILQR(prob, n).mpc(q[rows], xi[rows], pq[rows], px[rows], steps, t0=t0[rows], noise=noise[rows],
                                              pose_paths=paths[rows], **kw)
        for k in ("xs_q", "xs_xi", "us", "J", "max_violation", "mu", "pose_margin", "iters", "status"):
            assert torch.equal(bits(getattr(r, k)[rows]), bits(getattr(ra, k))), (k, rows)


# 7 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pose", "pose_paths", "box+pose_paths"])
def test_zero_penalty_is_the_unconstrained_loop(form):
    """test_gpu_mpc_constrained's test of this name with the pose family: with mu0 = 0 every multiplier and every I_mu stays zero,
    and zero terms change no bit of a solve (test_zero_multipliers_change_nothing, tests/test_gpu_pose_constraints.py)."""
    B, N, steps = 5, 20, 4
    prob, q, xi, pq, px, t0, noise, paths, kinds = workloads.se3_mpc_inspection(B, 8, N=N, seed=23)
    noise = noise[:, :steps]
    kw = dict(t0=t0, noise=noise, first_iters=6, iters_per_step=3, warm="states", check_every=0)
    s = BatchedTrackingILQR(prob, B)
    r0 = s.mpc(q, xi, pq, px, steps, **kw)
    con = dict(pose_constraints=paths[np.arange(B), t0]) if form == "pose" else dict(pose_paths=paths)
    if "box" in form:
        con.update(zip(("lb", "ub"), _box_of(r0)))
    r1 = s.mpc(q, xi, pq, px, steps, mu0=0.0, first_al_iters=1, al_iters_per_step=1, pose_kinds=kinds, **con, **kw)
    for k in ("xs_q", "xs_xi", "us", "J", "iters", "status"):
        assert torch.equal(bits(getattr(r0, k)), bits(getattr(r1, k))), k
    assert (r1.mu == 0).all() and r1.max_violation.shape == (B, steps) and r1.pose_margin.shape == (B, steps + 1)
    assert r0.max_violation is None and r0.pose_margin is None and r1.clearance is None


# 8 -------------------------------------------------------------------------------------------------------------------
def test_pose_slots_in_the_planner_reduce_the_violation():
    """Both loops run with the line search, and the constrained one caps mu at 1e3: the path leaves the cones for good, so the
    violation persists and mu grows at every step, and a step's few accept-always iterations diverge under a penalty that large
    (INTEGRATION.md 3m says the same of a box that starves the loop)."""
    B, N, steps = 8, 20, 20
    prob, q, xi, pq, px, t0, noise, paths, kinds = workloads.se3_mpc_inspection(B, steps, N=N, seed=24, sigma_noise=0.0)
    kw = dict(t0=t0, first_iters=30, iters_per_step=5, warm="states", check_every=0, line_search=True)
    s = BatchedTrackingILQR(prob, B)
    free = _margin(s.mpc(q, xi, pq, px, steps, **kw).xs_q, paths, t0, kinds).min(axis=1)
    print("unconstrained margin", free)
    assert (free < 0).all()  # a condition on the inputs: the unconstrained loop follows its path out of a cone in every trajectory
    r = s.mpc(q, xi, pq, px, steps, pose_paths=paths, pose_kinds=kinds, mu_max=1e3, **kw)
    con = host(r.pose_margin).min(axis=1)
    mv = host(r.max_violation)
    print("constrained margin", con, "max_violation first / last, batch mean", mv[:, 0].mean(), mv[:, -1].mean())
    assert np.allclose(host(r.pose_margin), _margin(r.xs_q, paths, t0, kinds), rtol=0, atol=1e-12)
    assert (con > free).all()  # the worst excursion is strictly smaller for every trajectory
    assert mv[:, -1].mean() < mv[:, 0].mean()


# 9 -------------------------------------------------------------------------------------------------------------------
def _fleet_slots(q_ref, c_tilt, c_view):
    """Per-knot slots [B, N+1, 2, 4] about per-trajectory references: a tilt cone about z, a view cone on the point 3 ahead of the
    reference's last pose"""
    B, N1 = q_ref.shape[:2]
    slots = np.empty((B, N1, 2, 4))
    slots[:, :, 0] = (0.0, 0.0, 1.0, c_tilt)
    slots[:, :, 1, :3] = (q_ref[:, -1, :3, 3] + 3.0 * q_ref[:, -1, :3, 0])[:, None]
    slots[:, :, 1, 3] = c_view
    return slots


def test_plan_fleet_with_pose_slots():
    F, G, N, sep = 2, 3, 20, 0.3
    B = F * G
    prob, q, xi, us, q_ref, xi_ref = workloads.se3_crossing_fleet(F, G, N=N, separation=sep)
    kinds = ("tilt_cone", "view_cone")
    tilt = q_ref[:, :, 2, 2]
    slots = _fleet_slots(q_ref, min(tilt.min() + 0.1, 0.9), 0.5)
    al = dict(n_al_iters=3, n_ilqr_iters=20, mu0=1.0, tol_constr=1e-3)
    s = BatchedTrackingILQR(prob, B)
    res, info = s.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, pose_constraints=slots, pose_kinds=kinds, **al)
    assert s._pose is None and s._obs is None
    assert (host(info["max_violation"]) > 0).any()  # the slots act
    # every round is al_fit_batch on its members' rows, the members before it as moving spheres
    s2, pos = BatchedTrackingILQR(prob, B), []
    for p in range(G):
        sl = slice(p, None, G)
        field = [np.concatenate([t, np.full((F, N + 1, 1), sep)], axis=-1)[:, :, None] for t in pos]
        obs = np.concatenate(field, axis=2) if pos else None
        r, i = s2.al_fit_batch(q[sl], xi[sl], us[sl], obstacles=obs, obstacle_kinds=None if obs is None else (0,) * p,
                               q_ref=q_ref[sl], xi_ref=xi_ref[sl], pose_constraints=slots[sl], pose_kinds=kinds, **al)
        for k in ("xs_q", "xs_xi", "us", "iters", "status"):
            assert torch.equal(bits(getattr(res, k)[sl]), bits(getattr(r, k))), (p, k)
        assert torch.equal(bits(info["max_violation"][sl]), bits(i["max_violation"])), p
        assert info["outer_iterations"][p] == i["outer_iterations"]
        pos.append(r.xs_q[:, :, :3, 3].cpu().numpy())
    # the other accepted shapes are the per-knot one
    rb, _ = s.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, pose_constraints=slots[:, 0], pose_kinds=kinds, **al)
    assert torch.equal(bits(rb.xs_q), bits(res.xs_q))
    # slots nobody violates, zero penalty: the plans of plan_fleet without them
    loose = _fleet_slots(q_ref, -0.999, -0.999)
    zero = dict(al, mu0=0.0, n_al_iters=2)
    r0, i0 = s.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, **zero)
    r1, i1 = s.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, pose_constraints=loose, pose_kinds=kinds, **zero)
    assert pose_margin(host(r1.xs_q), loose, kinds).min() > 0
    for k in ("xs_q", "xs_xi", "us", "iters", "status"):
        assert torch.equal(bits(getattr(r0, k)), bits(getattr(r1, k))), k
    # refused: kinds without slots, a family the caller attached
    with pytest.raises(ValueError):
        s.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, pose_kinds=kinds, **al)
    s3 = BatchedTrackingILQR(prob, B)  # (a handle that holds no references of a round's sub-batch)
    s3.set_al_pose_constraints(slots, kinds)
    with pytest.raises(ValueError, match="caller attached"):
        s3.plan_fleet(q, xi, us, q_ref, xi_ref, G, sep, pose_constraints=slots, pose_kinds=kinds, **al)
    s3.set_al_pose_constraints(None)


# 10 ------------------------------------------------------------------------------------------------------------------
def test_the_handle_is_left_clean_and_the_argument_errors():
    B, N, steps = 5, 20, 3
    prob, q, xi, pq, px, t0, noise, paths, kinds = workloads.se3_mpc_inspection(B, 8, N=N, seed=25)
    static = paths[np.arange(B), t0]
    fit = dict(mode="ms", n_iterations=5, check_every=0, **ZERO)
    fresh = BatchedTrackingILQR(prob, B).fit_batch(q, xi, None, **fit)
    s = BatchedTrackingILQR(prob, B)
    kw = dict(t0=t0, first_iters=4, iters_per_step=2, check_every=0)
    lb, ub = _box_of(s.mpc(q, xi, pq, px, steps, **kw))
    clean = lambda: s._al is None and s._obs is None and s._pose is None  # noqa: E731
    r = s.mpc(q, xi, pq, px, steps, lb=lb, ub=ub, pose_paths=paths, pose_kinds=kinds, **kw)
    assert clean() and r.pose_margin.shape == (B, steps + 1)
    assert_bitwise(fresh, s.fit_batch(q, xi, None, **fit), what="behind mpc")
    # paths on the solver's device are checked there and used as they are: the same loop, and a bad value is still refused
    d = torch.as_tensor(paths, **f64)
    seen = []
    rd = s.mpc(q, xi, pq, px, steps, lb=lb, ub=ub, pose_paths=d, pose_kinds=kinds,
               on_step=lambda t, out: seen.append(s._pose[0].data_ptr()), **kw)
    assert seen == [d.data_ptr()] * steps
    for k in ("xs_q", "us", "max_violation", "mu", "pose_margin"):
        assert torch.equal(bits(getattr(r, k)), bits(getattr(rd, k))), k
    bad = d.clone()
    bad[2, 1, 1, 3] = float("nan")
    with pytest.raises(ValueError):
        s.mpc(q, xi, pq, px, steps, pose_paths=bad, pose_kinds=kinds, **kw)
    assert clean()

    def stop(t, out):
        if t == 1:
            raise KeyError("stop")

    for con in (dict(pose_constraints=static), dict(pose_paths=paths, lb=lb, ub=ub)):
        with pytest.raises(KeyError):
            s.mpc(q, xi, pq, px, steps, pose_kinds=kinds, on_step=stop, **con, **kw)
        assert clean()
        assert_bitwise(fresh, s.fit_batch(q, xi, None, **fit), what="behind an mpc that raised")
    # the shared form is the per-trajectory one
    ra = s.mpc(q, xi, pq, px, steps, pose_constraints=static[0], pose_kinds=kinds, **kw)
    rb = s.mpc(q, xi, pq, px, steps, pose_constraints=np.ascontiguousarray(np.broadcast_to(static[0], static.shape)), pose_kinds=kinds, **kw)
    for k in ("xs_q", "us", "max_violation", "mu", "pose_margin"):
        assert torch.equal(bits(getattr(ra, k)), bits(getattr(rb, k))), k
    for bad in (dict(pose_constraints=static, pose_paths=paths, pose_kinds=kinds),      # both
                dict(pose_kinds=kinds),                                                   # kinds without slots
                dict(pose_paths=paths),                                                   # slots without kinds
                dict(pose_paths=paths, pose_kinds=kinds, mode="ss", warm="controls"),
                dict(pose_constraints=static, pose_kinds=kinds, mode="ss", warm="controls"),
                dict(pose_constraints=paths[:, :N + 1], pose_kinds=kinds),               # per knot: not static
                dict(pose_paths=paths[:4], pose_kinds=kinds), dict(pose_constraints=static[:4], pose_kinds=kinds),
                dict(pose_paths=paths[..., :3], pose_kinds=kinds), dict(pose_paths=paths[:, :1], pose_kinds=kinds),
                dict(pose_paths=paths, pose_kinds=kinds[:1]), dict(pose_paths=paths, pose_kinds=(0, 2)),
                dict(pose_paths=np.ones((B, 9, 9, 4)), pose_kinds=(0,) * 9),
                dict(pose_paths=paths, pose_kinds=kinds, first_al_iters=0)):
        with pytest.raises(ValueError):
            s.mpc(q, xi, pq, px, steps, **bad, **kw)
        assert clean()
    # a family the caller attached is still refused
    s.set_al_pose_constraints(static, kinds)
    with pytest.raises(ValueError, match="pose constraints"):
        s.mpc(q, xi, pq, px, steps, pose_paths=paths, pose_kinds=kinds, **kw)
    s.set_al_pose_constraints(None)
    assert_bitwise(fresh, s.fit_batch(q, xi, None, **fit), what="behind the refusals")
    # the SO3 family has no pose slots
    p3, q3, x3, _ = workloads.so3_tracking(2, N=N)
    path_q = np.broadcast_to(p3.q_ref, (2,) + p3.q_ref.shape)
    path_x = np.broadcast_to(p3.xi_ref, (2,) + p3.xi_ref.shape)
    s3 = BatchedTrackingILQR(p3, 2)
    for con in (dict(pose_constraints=static[:2]), dict(pose_paths=paths[:2])):
        with pytest.raises(ValueError, match="not offered"):
            s3.mpc(q3, x3, path_q, path_x, 2, pose_kinds=kinds, **con)
    assert s3._pose is None
