"""Synthetic workloads of the BASELINE.json configurations.

The reference paths (q_ref, xi_ref, dt) are the reference's own data files re-saved as .npz under
``data/`` (tests/golden/make_golden.py); everything else -- weights, nominal initial state, the
seeded perturbation of the batch -- follows the reference's benchmark scripts:
benchmark_SE3_tracking.py:67-79,175-190 and benchmark_drone_racing_tracking.py:56-66,168-210.
Pure NumPy host code (no solver arithmetic here).
"""
import os

import numpy as np

from .solver import TrackingProblem

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
SEED = 24234156  # the reference's seed constant (main_SE3ddp_tracking_exact.py:22)


def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])


def _so3_exp(w):
    th = np.linalg.norm(w)
    W = _skew(w)
    if th < 1e-8:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def _se3_exp(tau):
    w, v = tau[:3], tau[3:]
    th = np.linalg.norm(w)
    W = _skew(w)
    if th < 1e-8:
        V = np.eye(3) + 0.5 * W
    else:
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    T = np.eye(4)
    T[:3, :3] = _so3_exp(w)
    T[:3, 3] = V @ v
    return T


def _rot_zxy(z, x, y):
    """scipy Rotation.from_euler('zxy', [z, x, y], degrees=True).as_matrix(): lower-case axes are
    extrinsic rotations about the fixed z, then x, then y axes."""
    z, x, y = np.deg2rad([z, x, y])
    Rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1.0, 0], [-np.sin(y), 0, np.cos(y)]])
    return Ry @ Rx @ Rz


def load_reference(name):
    d = np.load(os.path.join(_DATA, "ref_%s.npz" % name))
    return d["q_ref"], d["xi_ref"], float(d["dt"])


def inertia():
    return np.diag([0.5, 0.7, 0.9, 1.0, 1.0, 1.0])


def perturbed_batch(q0, xi0, B, scale_pose, scale_twist, seed=SEED):
    """q0_b = q0 Exp(delta_b), xi0_b = xi0 + eta_b."""
    rng = np.random.default_rng(seed)
    x0_q = np.empty((B, 4, 4))
    x0_xi = np.empty((B, 6))
    for b in range(B):
        delta = rng.uniform(-1, 1, 6) * scale_pose
        eta = rng.uniform(-1, 1, 6) * scale_twist
        x0_q[b] = q0 @ _se3_exp(delta) if b > 0 else q0  # member 0 is the nominal problem
        x0_xi[b] = xi0 + (eta if b > 0 else 0)
    return x0_q, x0_xi


def _extend_reference(q_ref, xi_ref, dt, N):
    """Horizons beyond the stored 201 knots of path_se3_generate_sine_2 (the reference's longer problems --
    path_se3_spiral_static_velocity N = 400, the HEAD benchmark problem N = 955, benchmark_SE3_tracking.py:49-58 --
    are not among the stored data files): the path is continued the way the reference generates its own,
    q_{i+1} = q_i Exp(xi_i dt) with a smooth twist profile (main_SE3ddp_tracking_exact_ms.py:52-85), starting from
    the last stored knot.  Synthetic data of the reference's shape, not the reference's path."""
    n0 = q_ref.shape[0]
    q = np.empty((N + 1, 4, 4)); xi = np.empty((N + 1, 6))
    q[:n0] = q_ref; xi[:n0] = xi_ref
    for i in range(n0 - 1, N):
        s = float(i - (n0 - 1))
        xi[i + 1] = xi_ref[-1] + np.array([0.4 * np.sin(s / 40.0), 0.2 * np.sin(s / 55.0), 0.3 * np.sin(s / 70.0),
                                           0.5 * np.sin(s / 45.0), 0.4 * np.sin(s / 60.0), 0.3 * np.sin(s / 80.0)])
        q[i + 1] = q[i] @ _se3_exp(xi[i] * dt)
    return q, xi


def se3_tracking(B, N=200, R_scale=1e-5, seed=SEED):
    """BASELINE metric / config 3: SE3 exact tracking, N=200, dt=0.05 on path_se3_generate_sine_2."""
    q_ref, xi_ref, dt = load_reference("se3_sine2_n200")
    if N + 1 > q_ref.shape[0]:
        q_ref, xi_ref = _extend_reference(q_ref, xi_ref, dt, N)
    q_ref, xi_ref = q_ref[: N + 1], xi_ref[: N + 1]
    Q = np.diag([25.0, 25, 25, 10, 10, 10, 1, 1, 1, 1, 1, 1])
    prob = TrackingProblem("se3", inertia(), dt, Q, np.eye(6) * R_scale, 1.5 * Q, q_ref, xi_ref)
    q0 = np.eye(4)
    q0[:3, :3] = _rot_zxy(90.0, 10.0, 45.0)
    q0[:3, 3] = q_ref[0][:3, 3] - 1.0
    xi0 = np.ones(6) * 0.1
    x0_q, x0_xi = perturbed_batch(q0, xi0, B, np.array([0.3, 0.3, 0.3, 0.5, 0.5, 0.5]), 0.1, seed)
    return prob, x0_q, x0_xi, np.zeros((B, N, 6))


def drone_tracking(B, N=400, R_scale=1e-5, seed=SEED, perturb=1.0):
    """Config 5: DroneDynamics on the first N+1 knots of path_dense_random_columns_4obj (dt=0.004).
    `perturb` scales the spread of the initial states around the nominal one."""
    q_ref, xi_ref, dt = load_reference("drone_columns_n400")
    if not 1 <= N <= q_ref.shape[0] - 1:
        raise ValueError("path_dense_random_columns_4obj (stored part) has %d knots: horizon N must be in [1, %d]"
                         % (q_ref.shape[0], q_ref.shape[0] - 1))
    q_ref, xi_ref = q_ref[: N + 1], xi_ref[: N + 1]
    Q = np.diag([25.0, 25, 25, 10, 10, 10, 1, 1, 1, 1, 1, 1])
    prob = TrackingProblem("drone", inertia(), dt, Q, np.eye(4) * R_scale, 1.5 * Q, q_ref, xi_ref)
    q0 = np.eye(4)
    q0[:3, :3] = _rot_zxy(1e-4, 0.0, 0.0)
    q0[:3, 3] = q_ref[0][:3, 3] - 0.1
    xi0 = np.ones(6) * 1e-3
    x0_q, x0_xi = perturbed_batch(q0, xi0, B, perturb * 0.1 * np.array([0.3, 0.3, 0.3, 0.5, 0.5, 0.5]), perturb * 0.01, seed)
    return prob, x0_q, x0_xi, np.zeros((B, N, 4))


def pendulum_swingup(B, xi0_scale=5.0, seed=SEED):
    """Pendulum3dDyanmics swing-up tracking (main_pendulum3d_ddp_tracking_exact_ms.py:40-122,
    benchmark_pendulum_swingup.py:50-72): path_3dpendulum_swingup (N=80, dt=0.025), J=diag(.5,.7,.9), m=1,
    length=.5, Q=diag(10,10,10,1,1,1), P=10Q, R=1e-2 I3, q0 = from_euler('xy',[10,45] deg),
    xi0 = (1,1,0)*xi0_scale (5 in the main script, 1 in the benchmark)."""
    from .solver import embed_pendulum3d
    R_ref, w_ref, dt = load_reference("pendulum_swingup_n80")
    Q6 = np.diag([10.0, 10, 10, 1, 1, 1])
    prob = embed_pendulum3d(np.diag([0.5, 0.7, 0.9]), 1.0, 0.5, dt, Q6, np.eye(3) * 1e-2, 10 * Q6, R_ref, w_ref)
    x, y = np.deg2rad([10.0, 45.0])
    Rx = np.array([[1.0, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1.0, 0], [-np.sin(y), 0, np.cos(y)]])
    q0 = np.eye(4)
    q0[:3, :3] = Ry @ Rx  # extrinsic x then y
    xi0 = np.array([1.0, 1.0, 0.0, 0, 0, 0]) * xi0_scale
    x0_q, x0_xi = perturbed_batch(q0, xi0, B, np.array([0.3, 0.3, 0.3, 0, 0, 0]), np.array([0.1, 0.1, 0.1, 0, 0, 0]), seed)
    return prob, x0_q, x0_xi, np.zeros((B, prob.N, 6))


def so3_tracking(B=1, N=100, seed=SEED):
    """Config 2: SO3 exact tracking (main_SO3ddp_tracking_exact.py:75-125): first N+1 knots of
    path_3dpendulum_8shape (dt=.04), J=diag(.5,.7,.9), Q=diag(10,10,10,1,1,1), P=10Q, R=1e-5 I3,
    x0 = (q_ref[0], xi_ref[0]); members b > 0 are perturbed in rotation / angular velocity."""
    from .solver import embed_so3
    R_ref, w_ref, dt = load_reference("so3_8shape_n249")
    if not 1 <= N <= R_ref.shape[0] - 1:
        raise ValueError("path_3dpendulum_8shape has %d knots: horizon N must be in [1, %d]"
                         % (R_ref.shape[0], R_ref.shape[0] - 1))
    R_ref, w_ref = R_ref[: N + 1], w_ref[: N + 1]
    Q6 = np.diag([10.0, 10, 10, 1, 1, 1])
    prob = embed_so3(np.diag([0.5, 0.7, 0.9]), dt, Q6, np.eye(3) * 1e-5, 10 * Q6, R_ref, w_ref)
    q0 = np.eye(4)
    q0[:3, :3] = R_ref[0]
    xi0 = np.r_[w_ref[0], 0, 0, 0]
    x0_q, x0_xi = perturbed_batch(q0, xi0, B, np.array([0.3, 0.3, 0.3, 0, 0, 0]), np.array([0.1, 0.1, 0.1, 0, 0, 0]), seed)
    return prob, x0_q, x0_xi, np.zeros((B, N, 6))


def al_tracking(B, N=200, seed=SEED):
    """Config 4: SE3 AL-DDP multiple shooting with input box constraints
    (main_SE3ddp_tracking_exact_al_ms.py:47-152): constant-twist reference xi_ref=[0,0,1,2,0,.2], dt=.01,
    Q=diag(10,10,10,1,...,1), P=10Q, R=0, InputConstraint(-10,10), nominal x0=[I,(-1,-1,-.2)],
    xi0=[0,0,.1,2,0,.2].  Returns (prob, x0_q, x0_xi, us_init, lb, ub)."""
    dt = 0.01
    xi_c = np.array([0.0, 0.0, 1.0, 2.0, 0.0, 0.2])
    step = _se3_exp(xi_c * dt)
    q_ref = np.empty((N + 1, 4, 4))
    q_ref[0] = np.eye(4)
    for i in range(N):
        q_ref[i + 1] = q_ref[i] @ step
    xi_ref = np.repeat(xi_c[None], N + 1, 0)
    Q = np.diag([10.0, 10, 10, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    prob = TrackingProblem("se3", inertia(), dt, Q, np.zeros((6, 6)), 10 * Q, q_ref, xi_ref)
    q0 = np.eye(4)
    q0[:3, 3] = [-1.0, -1.0, -0.2]
    xi0 = np.array([0.0, 0.0, 0.1, 2.0, 0.0, 0.2])
    x0_q, x0_xi = perturbed_batch(q0, xi0, B, 0.3 * np.array([0.3, 0.3, 0.3, 0.5, 0.5, 0.5]), 0.05, seed)
    return prob, x0_q, x0_xi, np.zeros((B, N, 6)), -10.0 * np.ones(6), 10.0 * np.ones(6)


def rigid_motions(R, seed=SEED, angle=np.pi, shift=2.0):
    """R seeded rigid motions G_r = Exp([w; v]): w uniform in the ball of radius `angle` by axis and angle, v uniform in
    [-shift, shift]^3 (the translation part of G_r is V(w) v)."""
    rng = np.random.default_rng(seed)
    G = np.empty((R, 4, 4))
    for r in range(R):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        G[r] = _se3_exp(np.r_[ax * rng.uniform(0.0, angle), rng.uniform(-shift, shift, 3)])
    return G


def se3_multiref(B, R, N=200, index=None, seed=SEED):
    """B trajectories tracking R distinct references: reference r is path_se3_generate_sine_2 (se3_tracking's path) moved
    by the rigid motion G_r, q_ref_r[i] = G_r q_ref[i], with the same body twists xi_ref -- the same motion seen from
    another frame, so each reference stays kinematically consistent.  Trajectory b tracks reference index[b] (default
    b % R) and starts where se3_tracking places member b, moved by the same G_r: relative to its own reference's first
    pose.  Returns (prob, x0_q, x0_xi, us0, q_ref [B, N+1, 4, 4], xi_ref [B, N+1, 6], index [B], G [R, 4, 4]); prob is
    se3_tracking's problem (its shared reference is the unmoved path)."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    index = np.arange(B) % R if index is None else np.asarray(index, dtype=np.int64)
    if index.shape != (B,) or index.min() < 0 or index.max() >= R:
        raise ValueError("index must hold B = %d reference numbers in [0, %d)" % (B, R))
    G = rigid_motions(R, seed=seed + 1)
    q_refs = np.einsum("rab,ibc->riac", G, prob.q_ref)
    q_ref = q_refs[index]
    xi_ref = np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape).copy()
    x0_q = np.einsum("bac,bcd->bad", G[index], x0_q)
    return prob, x0_q, x0_xi, us0, q_ref, xi_ref, index, G


def se3_weight_sweep(B, K, N=200, spread=3.0, seed=SEED):
    """B trajectories of se3_tracking's workload under K diagonal weight sets: set k scales each diagonal entry of the
    headline Q, P and R by its own factor, log-uniform in [1/spread, spread] (seeded; set 0 as well).  Trajectory b uses set
    b % K.  Returns (prob, x0_q, x0_xi, us0, Q [B, 12, 12], P [B, 12, 12], R [B, 6, 6], index [B], (Qk [K, 12, 12],
    Pk [K, 12, 12], Rk [K, 6, 6])); prob is se3_tracking's problem with its shared weights."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    rng = np.random.default_rng(seed + 2)
    ls = np.log(spread)
    qd, pd, rd = np.diag(prob.Q), np.diag(prob.P), np.diag(prob.R)
    Qk = np.stack([np.diag(qd * np.exp(rng.uniform(-ls, ls, 12))) for _ in range(K)])
    Pk = np.stack([np.diag(pd * np.exp(rng.uniform(-ls, ls, 12))) for _ in range(K)])
    Rk = np.stack([np.diag(rd * np.exp(rng.uniform(-ls, ls, 6))) for _ in range(K)])
    index = np.arange(B) % K
    return prob, x0_q, x0_xi, us0, Qk[index], Pk[index], Rk[index], index, (Qk, Pk, Rk)


def gate_knots(N, gates):
    """The knots of `gates` gates spread evenly inside the horizon: round((g + 1) N / (gates + 1)), g = 0 .. gates-1."""
    if not 1 <= gates < N:
        raise ValueError("gates must be in 1..N-1")
    k = np.rint((np.arange(gates) + 1.0) * N / (gates + 1.0)).astype(np.int64)
    if len(np.unique(k)) != gates or k[0] < 1 or k[-1] > N - 1:
        raise ValueError("%d gates do not fit %d knots" % (gates, N))
    return k


def se3_gates(B, N=200, gates=3, gate_gain=64.0, seed=SEED):
    """Gates on se3_tracking's path: the pose is tracked loosely (pose weights a hundredth of se3_tracking's, Q = diag(0.25 x 3,
    0.1 x 3, 1 x 6), P = 1.5 Q) except at `gates` gate knots, where a pose schedule multiplies the pose weights by gate_gain:
    pass the gates tightly, track loosely between them.  The gates of member 0 sit at gate_knots(N, gates); those of the other
    members are moved by up to a quarter of the gate spacing (at most two knots) either way, seeded, so that every trajectory
    has its own schedule.  The reference passes through every gate: q_ref at a gate knot is the gate's pose.
    Returns (prob, x0_q, x0_xi, us0, pose_scale [B, N+1, 6], knots [B, gates]): fit_batch(x0_q, x0_xi, us0,
    pose_scale=pose_scale) on a solver for prob; pose_scale is 1 everywhere and gate_gain at the gate knots."""
    base, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    Q = np.diag([0.25, 0.25, 0.25, 0.1, 0.1, 0.1, 1, 1, 1, 1, 1, 1])
    prob = TrackingProblem("se3", base.J, base.dt, Q, base.R, 1.5 * Q, base.q_ref, base.xi_ref)
    k0 = gate_knots(N, gates)
    jitter = min(2, (N // (gates + 1)) // 4)
    rng = np.random.default_rng(seed + 5)
    knots = k0[None, :] + rng.integers(-jitter, jitter + 1, size=(B, gates))
    knots[0] = k0
    pose_scale = np.ones((B, N + 1, 6))
    pose_scale[np.arange(B)[:, None], knots] = float(gate_gain)
    return prob, x0_q, x0_xi, us0, pose_scale, knots


def se3_policy_eval(B, S, N=200, sigma_pose=0.05, sigma_twist=0.05, sigma_noise=0.01, seed=SEED):
    """Monte-Carlo inputs for the closed loop of se3_tracking's workload (BatchedTrackingILQR.policy_rollout): S seeded
    perturbations per trajectory.  Returns (prob, x0_q, x0_xi, us0, dx0 [B, S, 12], noise [B, S, N, 6]); dx0 is Gaussian
    in the error coordinates of the gains, sigma_pose on the pose part (rotation, translation), sigma_twist on the twist,
    and noise is a Gaussian twist disturbance with sigma_noise behind every step."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    rng = np.random.default_rng(seed + 3)
    dx0 = np.concatenate([rng.normal(0.0, sigma_pose, (B, S, 6)), rng.normal(0.0, sigma_twist, (B, S, 6))], axis=2)
    noise = rng.normal(0.0, sigma_noise, (B, S, N, 6))
    return prob, x0_q, x0_xi, us0, dx0, noise


def drone_actuated(B, S, N=400, tau=0.03, rate=None, delay=1, sigma_pose=0.05, sigma_twist=0.05, sigma_noise=0.01, seed=SEED):
    """drone_tracking's workload with se3_policy_eval's perturbations and a motor model (policy_rollout(act_*=)): a first-order
    lag of tau seconds (30 ms, 7.5 knots at dt = 0.004) on every input, a transport delay of `delay` knots and a slew limit of
    `rate` units per second per input -- None: the thrust may cross four times its hover value (mass x 9.81) in a second, each
    torque 2 units.  Returns (prob, x0_q, x0_xi, us0, dx0 [B, S, 12], noise [B, S, N, 6], act) with act the keywords
    dict(act_tau=, act_rate=, act_delay=)."""
    prob, x0_q, x0_xi, us0 = drone_tracking(B, N=N, seed=seed)
    rng = np.random.default_rng(seed + 3)
    dx0 = np.concatenate([rng.normal(0.0, sigma_pose, (B, S, 6)), rng.normal(0.0, sigma_twist, (B, S, 6))], axis=2)
    noise = rng.normal(0.0, sigma_noise, (B, S, N, 6))
    if rate is None:
        rate = np.array([2.0, 2.0, 2.0, 4.0 * 9.81 * float(prob.J[3, 3])])
    act = dict(act_tau=np.full(4, float(tau)), act_rate=np.broadcast_to(np.asarray(rate, float), (4,)).copy(), act_delay=int(delay))
    return prob, x0_q, x0_xi, us0, dx0, noise, act


def se3_gain_sweep_actuated(B, S, N=200, centre=0.1, spread=10.0, tau=0.03, delay=1, sigma_pose=0.02, sigma_twist=0.02,
                            sigma_noise=0.002, seed=SEED):
    """A weight sweep on se3_tracking's workload (se3_weight_sweep's shape) along ONE direction, the loop gain: member b scales
    Q and P by g_b and R by 1 / g_b, g log-spaced from centre / spread (member 0) to centre spread (member B - 1), so that the
    feedback gains grow with b.  Without an actuator nothing tells the members apart but their weights: every one of them
    tracks, and the analytic companions (policy_value, policy_covariance) describe that loop.  Behind a 30 ms motor (a lag of
    tau seconds, 0.6 knots at dt = 0.05) and a delay of `delay` knots the low-gain half barely notices (J up by a few per
    cent) while the high-gain half loses its phase margin: J rises by tens of per cent and the top of the sweep leaves the
    finite numbers.  Every member is costed with ITS OWN weights, so a member is compared with itself, with and without the
    actuator.
    Returns (prob, x0_q, x0_xi, us0, Q [B, 12, 12], P [B, 12, 12], R [B, 6, 6], gain [B], high [B] bool -- the upper half of
    the sweep --, dx0 [B, S, 12], noise [B, S, N, 6], act) with act = dict(act_tau=, act_delay=).  Every member starts from
    the same state, member 0's."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, R_scale=1e-3, seed=seed)
    x0_q = np.repeat(np.asarray(x0_q)[:1], B, axis=0)
    x0_xi = np.repeat(np.asarray(x0_xi)[:1], B, axis=0)
    gain = float(centre) * (np.exp(np.linspace(-np.log(spread), np.log(spread), B)) if B > 1 else np.ones(1))
    Q = gain[:, None, None] * prob.Q[None]
    P = gain[:, None, None] * prob.P[None]
    R = prob.R[None] / gain[:, None, None]
    high = np.arange(B) >= (B + 1) // 2
    rng = np.random.default_rng(seed + 3)
    dx0 = np.concatenate([rng.normal(0.0, sigma_pose, (B, S, 6)), rng.normal(0.0, sigma_twist, (B, S, 6))], axis=2)
    noise = rng.normal(0.0, sigma_noise, (B, S, N, 6))
    act = dict(act_tau=np.full(6, float(tau)), act_delay=int(delay))
    return prob, x0_q, x0_xi, us0, Q, P, R, gain, high, dx0, noise, act


def se3_covariance(B, N=200, sigma_pose=0.05, sigma_twist=0.05, sigma_noise=0.01, seed=SEED):
    """Covariance inputs for the closed loop of se3_tracking's workload (BatchedTrackingILQR.policy_covariance), the analytic
    counterpart of se3_policy_eval's samples.  Returns (prob, x0_q, x0_xi, us0, Sigma0 [B, 12, 12], W [B, 6, 6]): seeded, per
    trajectory and not diagonal -- each is Q D Q^T with a random rotation Q (the orthogonal factor of a Gaussian matrix) of a
    diagonal D whose standard deviations are sigma_pose (pose part) and sigma_twist (twist part) resp. sigma_noise, each
    scaled by a factor drawn uniformly from [0.5, 1.5].  A sigma of zero gives a zero matrix."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    rng = np.random.default_rng(seed + 5)

    def rotated(sig):
        n = sig.shape[0]
        out = np.zeros((B, n, n))
        for b in range(B):
            Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
            d = (sig * rng.uniform(0.5, 1.5, n)) ** 2
            out[b] = (Q * d) @ Q.T
            out[b] = 0.5 * (out[b] + out[b].T)
        return out

    Sigma0 = rotated(np.r_[[float(sigma_pose)] * 6, [float(sigma_twist)] * 6])
    W = rotated(np.full(6, float(sigma_noise)))
    return prob, x0_q, x0_xi, us0, Sigma0, W


def se3_estimated(B, N=200, sigma_pose=0.05, sigma_twist=0.05, sigma_noise=0.01, seed=SEED):
    """Output-feedback inputs for the closed loop of se3_tracking's workload (BatchedTrackingILQR.policy_covariance_estimated):
    se3_covariance's (prob, x0_q, x0_xi, us0, Sigma0, W) plus seeded measurement-noise variances V [B, 12] =
    diag(Sigma0) * U[0.25, 4] -- a sensor between twice as good and twice as bad, in standard deviation, as the start
    knowledge of each coordinate.  Which coordinates are measured (the mask) is the caller's choice; a Sigma0 of zero gives
    V = 0, which no coordinate may then be measured with."""
    prob, x0_q, x0_xi, us0, Sigma0, W = se3_covariance(B, N=N, sigma_pose=sigma_pose, sigma_twist=sigma_twist,
                                                       sigma_noise=sigma_noise, seed=seed)
    rng = np.random.default_rng(seed + 9)
    V = np.einsum("bii->bi", Sigma0) * rng.uniform(0.25, 4.0, (B, 12))
    return prob, x0_q, x0_xi, us0, Sigma0, W, V


def plant_mismatch(B, S, kind="se3", N=None, sigma_inertia=0.1, sigma_mass=0.1, rotate=False, seed=SEED):
    """Model-mismatch inputs for the closed loop (BatchedTrackingILQR.policy_rollout with plant_J): se3_policy_eval's
    perturbations on se3_tracking's (kind="se3", N default 200) or drone_tracking's (kind="drone", N default 400) workload,
    plus a seeded plant per sample.  Returns (prob, x0_q, x0_xi, us0, dx0 [B, S, 12], noise [B, S, N, 6], plant_J
    [B, S, 6, 6]).  Plant (b, s) is blkdiag(Ib, m I3) with the model's principal moments and mass each scaled by exp(N(0,
    sigma_inertia^2)) resp. exp(N(0, sigma_mass^2)); rotate=True turns Ib into R diag R^T with a uniformly random rotation R
    (dense blocks), else Ib stays diagonal."""
    if kind not in ("se3", "drone"):
        raise ValueError("kind must be 'se3' or 'drone'")
    if kind == "se3":
        prob, x0_q, x0_xi, us0 = se3_tracking(B, N=200 if N is None else N, seed=seed)
    else:
        prob, x0_q, x0_xi, us0 = drone_tracking(B, N=400 if N is None else N, seed=seed)
    n = prob.N
    rng = np.random.default_rng(seed + 5)
    dx0 = np.concatenate([rng.normal(0.0, 0.05, (B, S, 6)), rng.normal(0.0, 0.05, (B, S, 6))], axis=2)
    noise = rng.normal(0.0, 0.01, (B, S, n, 6))
    J0 = np.asarray(prob.J, dtype=np.float64)
    moments = np.diag(J0)[:3] * np.exp(rng.normal(0.0, sigma_inertia, (B, S, 3)))
    mass = J0[4, 4] * np.exp(rng.normal(0.0, sigma_mass, (B, S)))
    plant_J = np.zeros((B, S, 6, 6))
    for b in range(B):
        for s in range(S):
            Ib = np.diag(moments[b, s])
            if rotate:
                q = rng.normal(size=4)
                q /= np.linalg.norm(q)
                w, x, y, z = q
                R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                              [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                              [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
                Ib = R @ Ib @ R.T
                Ib = 0.5 * (Ib + Ib.T)
            plant_J[b, s, :3, :3] = Ib
            plant_J[b, s, 3:, 3:] = mass[b, s] * np.eye(3)
    return prob, x0_q, x0_xi, us0, dx0, noise, plant_J


def se3_mpc(B, steps, N=200, T=None, R=4, sigma_pose=0.05, sigma_twist=0.05, sigma_noise=0.01, seed=SEED):
    """Receding-horizon inputs (BatchedTrackingILQR.mpc) on se3_tracking's model: B trajectories, each following its own
    path of T+1 knots (default T = N + steps) -- se3_tracking's path continued to T knots (_extend_reference) and moved by
    one of R rigid motions (rigid_motions), as se3_multiref does -- from its own phase t0 in [0, T // 4).  Trajectory b
    starts near knot t0[b] of its path (pose Exp-perturbed with sigma_pose, twist with sigma_twist), and a Gaussian twist
    disturbance with sigma_noise follows every step.  Returns (prob, x0_q [B, 4, 4], x0_xi [B, 6], path_q [B, T+1, 4, 4],
    path_xi [B, T+1, 6], t0 [B] int32, noise [B, steps, 6]); prob's shared reference is the first N+1 knots of the unmoved
    path."""
    prob, _, _, _ = se3_tracking(1, N=N, seed=seed)
    T = N + steps if T is None else int(T)
    q_ref, xi_ref, dt = load_reference("se3_sine2_n200")
    if T + 1 > q_ref.shape[0]:
        q_ref, xi_ref = _extend_reference(q_ref, xi_ref, dt, T)
    q_ref, xi_ref = q_ref[: T + 1], xi_ref[: T + 1]
    G = rigid_motions(R, seed=seed + 1)
    index = np.arange(B) % R
    path_q = np.einsum("bac,icd->biad", G[index], q_ref)
    path_xi = np.broadcast_to(xi_ref, (B,) + xi_ref.shape).copy()
    rng = np.random.default_rng(seed + 4)
    t0 = rng.integers(0, max(T // 4, 1), B).astype(np.int32)
    x0_q = np.empty((B, 4, 4))
    for b in range(B):
        x0_q[b] = path_q[b, t0[b]] @ _se3_exp(rng.normal(0.0, sigma_pose, 6))
    x0_xi = path_xi[np.arange(B), t0] + rng.normal(0.0, sigma_twist, (B, 6))
    noise = rng.normal(0.0, sigma_noise, (B, steps, 6))
    return prob, x0_q, x0_xi, path_q, path_xi, t0, noise


def se3_mpc_estimated(B, steps, N=200, sigma_est=0.02, sigma_meas=0.01, seed=SEED, **mpc_kw):
    """Output-feedback receding-horizon inputs (BatchedTrackingILQR.mpc with meas_* / est_*): se3_mpc's
    (prob, x0_q, x0_xi, path_q, path_xi, t0, noise) -- x0 is now what the vehicle BELIEVES -- plus a dict of the seeded
    keywords of the estimated loop: est_Sigma0 [B, 12, 12] = diag(sigma_est^2 U[0.5, 1.5]^2), the initial belief's covariance;
    est_dx0 [B, 12] ~ N(0, est_Sigma0), where the true state starts relative to the belief; est_W [B, 6, 6] = sigma_noise^2 I,
    the covariance se3_mpc draws its twist disturbance from; meas_V [B, 12] = sigma_meas^2 U[0.25, 4] and meas_noise
    [B, steps+1, 12] ~ N(0, meas_V).  Which coordinates are measured (meas_mask) is the caller's choice."""
    sigma_noise = mpc_kw.get("sigma_noise", 0.01)
    prob, x0_q, x0_xi, path_q, path_xi, t0, noise = se3_mpc(B, steps, N=N, seed=seed, **mpc_kw)
    rng = np.random.default_rng(seed + 13)
    sd = sigma_est * rng.uniform(0.5, 1.5, (B, 12))
    Sigma0 = np.zeros((B, 12, 12))
    Sigma0[:, np.arange(12), np.arange(12)] = sd ** 2
    dx0 = rng.normal(size=(B, 12)) * sd
    W = np.broadcast_to(np.eye(6) * float(sigma_noise) ** 2, (B, 6, 6)).copy()
    V = float(sigma_meas) ** 2 * rng.uniform(0.25, 4.0, (B, 12))
    meas_noise = rng.normal(size=(B, steps + 1, 12)) * np.sqrt(V)[:, None, :]
    est = dict(meas_V=V, meas_noise=meas_noise, est_Sigma0=Sigma0, est_W=W, est_dx0=dx0)
    return prob, x0_q, x0_xi, path_q, path_xi, t0, noise, est


def _obstacle_field(q_ref, B, K, r_lo, r_hi, seed):
    """K seeded keep-out spheres per trajectory on its reference path: sphere k of trajectory b is centred on the reference
    position of a knot drawn from the middle half of the horizon (ordered, one per K-th of it), moved by at most 0.3 r, with a
    radius r uniform in [r_lo, r_hi].  The path passes through every sphere, so the unconstrained tracking optimum violates
    them; the start and the end of the path stay clear.  Returns obstacles [B, K, 4] rows (cx, cy, cz, r)."""
    q_ref = np.asarray(q_ref)
    N = q_ref.shape[-3] - 1
    rng = np.random.default_rng(seed)
    obs = np.empty((B, K, 4))
    lo, span = N // 4, max(1, N // 2)
    for b in range(B):
        t = (q_ref[b] if q_ref.ndim == 4 else q_ref)[:, :3, 3]
        for k in range(K):
            i = lo + int(rng.integers(k * span // K, max(k * span // K + 1, (k + 1) * span // K)))
            r = rng.uniform(r_lo, r_hi)
            d = rng.normal(size=3)
            obs[b, k, :3] = t[i] + 0.3 * r * rng.uniform() * d / np.linalg.norm(d)
            obs[b, k, 3] = r
    return obs


def se3_obstacle_field(B, K, N=200, seed=SEED):
    """se3_tracking's workload with K keep-out spheres per trajectory on its reference path (_obstacle_field; radii 0.2 .. 0.4,
    two to four knots of the path), different for every trajectory.  Returns (prob, x0_q, x0_xi, us0, obstacles [B, K, 4])."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    return prob, x0_q, x0_xi, us0, _obstacle_field(prob.q_ref, B, K, 0.2, 0.4, seed + 3)


def drone_obstacle_field(B, K, N=400, seed=SEED):
    """The drone variant (config 5, drone_tracking's workload) with K keep-out spheres per trajectory on the racing path
    (_obstacle_field; radii 0.1 .. 0.2, four to eight knots of the path: the drone tracks its path loosely, and a smaller
    sphere would hardly be violated).  Returns (prob, x0_q, x0_xi, us0, obstacles [B, K, 4])."""
    prob, x0_q, x0_xi, us0 = drone_tracking(B, N=N, seed=seed)
    return prob, x0_q, x0_xi, us0, _obstacle_field(prob.q_ref, B, K, 0.1, 0.2, seed + 3)


DERATED_SPAN = np.array([300.0, 450.0, 40.0, 30.0])  # the free solve's input range at R_scale = 1e-3: torques, thrust
DERATED_CENTRE = np.array([0.0, 0.0, 0.0, 15.0])


def drone_derated(B, N=400, tight=0.5, wide=4.0, derate=0.5, seed=SEED):
    """A drone fleet whose members have different actuators, each derated mid-flight: drone_tracking's workload (R = 1e-3 I)
    with an input box per trajectory and knot (al_fit_batch(lb=, ub=), [B, N, m]).  Trajectory b's box is DERATED_CENTRE +-
    w_b DERATED_SPAN with w_b spaced geometrically from `tight` (binds hard on the roll and pitch torques) to `wide` (never
    binds) and shuffled by the seed; from knot N // 2 on every width is `derate` times that (a derating that starts
    mid-horizon: the narrow members then bind there as well).  Returns (prob, x0_q, x0_xi, us0, lb, ub, width [B])."""
    prob, x0_q, x0_xi, us0 = drone_tracking(B, N=N, R_scale=1e-3, seed=seed)
    w = tight * (wide / tight) ** (np.arange(B) / max(B - 1, 1))
    w = w[np.random.default_rng(seed + 11).permutation(B)]
    half = w[:, None, None] * DERATED_SPAN[None, None, :] * np.where(np.arange(N) >= N // 2, derate, 1.0)[None, :, None]
    return prob, x0_q, x0_xi, us0, DERATED_CENTRE - half, DERATED_CENTRE + half, w


CORRIDOR_KINDS = ("half_space", "half_space", "keep_in", "column", "column", "sphere")


def _corridor(q_ref, x0_q, r_lo, r_hi, seed):
    """The six slots of a flight corridor per trajectory (kinds CORRIDOR_KINDS, tolg_set_al_obstacle_kinds), laid over the
    middle half of the reference path so that the path breaks each of them while the start x0 of every trajectory keeps them:
      floor    (0, 0, -1, -z_f): z >= z_f, a quarter of the middle half's height above its lowest knot, but below the start;
      ceiling  (0, 0, 1, z_c):   z <= z_c, a quarter of that height below its highest knot, but above the start;
      geofence of radius D, the distance from the start to the knot p furthest from it, centred 0.05 D behind the start on
               the line from p: the start lies deep inside and p 0.05 D outside;
      two columns through knots of the second and third quarter, radius in [r_lo, r_hi] and at most half the horizontal
               distance to the start;
      one keep-out sphere of _obstacle_field.
    Returns obstacles [B, 6, 4]."""
    t = np.asarray(q_ref)[:, :3, 3]
    N = t.shape[0] - 1
    B = x0_q.shape[0]
    rng = np.random.default_rng(seed)
    mid = t[N // 4: N // 4 + max(2, N // 2)]
    zlo, zhi = mid[:, 2].min(), mid[:, 2].max()
    h = zhi - zlo
    obs = np.empty((B, 6, 4))
    obs[:, 5] = _obstacle_field(q_ref, B, 1, r_lo, r_hi, seed + 1)[:, 0]
    for b in range(B):
        s = np.asarray(x0_q[b]).reshape(4, 4)[:3, 3]
        obs[b, 0] = (0.0, 0.0, -1.0, -min(zlo + 0.25 * h, s[2] - 0.1 * h))
        obs[b, 1] = (0.0, 0.0, 1.0, max(zhi - 0.25 * h, s[2] + 0.1 * h))
        p = mid[np.argmax(np.linalg.norm(mid - s, axis=1))]
        D = np.linalg.norm(p - s)
        obs[b, 2, :3], obs[b, 2, 3] = s - 0.05 * (p - s), D
        for k in range(2):
            c = mid[int(rng.integers(k * len(mid) // 2, (k + 1) * len(mid) // 2))]
            r = min(rng.uniform(r_lo, r_hi), 0.5 * np.linalg.norm(c[:2] - s[:2]))
            obs[b, 3 + k] = (c[0], c[1], 0.0, r)
    return obs


def se3_corridor(B, N=200, seed=SEED):
    """se3_tracking's workload inside a flight corridor of six slots of four kinds (_corridor: floor, ceiling, geofence, two
    columns of radius 0.15 .. 0.3, one keep-out sphere), different for every trajectory; the unconstrained tracking optimum
    breaks them.  Returns (prob, x0_q, x0_xi, us0, obstacles [B, 6, 4], kinds): what al_fit_batch(obstacles=,
    obstacle_kinds=) takes."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, seed=seed)
    return prob, x0_q, x0_xi, us0, _corridor(prob.q_ref, x0_q, 0.15, 0.3, seed + 7), CORRIDOR_KINDS


INSPECTION_KINDS = ("tilt_cone", "view_cone")


def se3_inspection(B, N=200, seed=SEED):
    """se3_tracking's workload (R_scale 1e-3) under two pose constraints per trajectory (kinds INSPECTION_KINDS,
    tolg_set_al_pose_constraints), given per knot:
      a tilt cone about world z, (0, 0, 1, c): c lies 0.2 above the smallest n^T R e3 of the reference path (and at most
               0.9), so the path's most tilted knots leave the cone by up to 0.2 while every start, all far more upright,
               is inside;
      a view cone on a target that drifts per knot, (p_i, c): p_i moves on a line from 3 ahead of trajectory b's own start
               pose (along its forward axis: on the cone's axis at knot 0) to 3 ahead of the reference's last pose, bent
               sideways by a seeded offset of up to 0.5; c lies a fifth of the way from the smallest e1^T b / |b| of the
               second half of the reference path under that target to 1, so the path leaves the cone where it looks
               furthest away, on a stretch that a solve from the trajectory's own start has reached.
    The reference path leaves both cones in every trajectory; the start of every trajectory satisfies both.  Returns (prob,
    x0_q, x0_xi, us0, slots [B, N+1, 2, 4], kinds): what al_fit_batch(pose_constraints=, pose_kinds=) takes."""
    prob, x0_q, x0_xi, us0 = se3_tracking(B, N=N, R_scale=1e-3, seed=seed)
    rng = np.random.default_rng(seed + 9)
    R, t = prob.q_ref[:, :3, :3], prob.q_ref[:, :3, 3]
    slots = np.empty((B, N + 1, 2, 4))
    slots[:, :, 0] = (0.0, 0.0, 1.0, min(R[:, 2, 2].min() + 0.2, 0.9))
    s = np.linspace(0.0, 1.0, N + 1)[:, None]
    for b in range(B):
        X0 = np.asarray(x0_q[b]).reshape(4, 4)
        p0, p1 = X0[:3, 3] + 3.0 * X0[:3, 0], t[N] + 3.0 * R[N][:, 0]
        p = (1.0 - s) * p0 + s * p1 + np.sin(np.pi * s) * rng.uniform(-0.5, 0.5, 3)
        bv = np.einsum("iac,ia->ic", R, p - t)
        cv = bv[:, 0] / np.linalg.norm(bv, axis=1)
        late = cv[N // 2:].min()   # (the second half: where a solve from the trajectory's own start has reached the path)
        slots[b, :, 1, :3], slots[b, :, 1, 3] = p, late + 0.2 * (1.0 - late)
    return prob, x0_q, x0_xi, us0, slots, INSPECTION_KINDS


def drone_corridor(B, N=400, seed=SEED):
    """The drone variant (drone_tracking's workload) of se3_corridor, columns and sphere of radius 0.08 .. 0.15.  Returns
    (prob, x0_q, x0_xi, us0, obstacles [B, 6, 4], kinds)."""
    prob, x0_q, x0_xi, us0 = drone_tracking(B, N=N, seed=seed)
    return prob, x0_q, x0_xi, us0, _corridor(prob.q_ref, x0_q, 0.08, 0.15, seed + 7), CORRIDOR_KINDS


def se3_moving_obstacle_field(B, K, N=200, seed=SEED):
    """se3_obstacle_field's workload with its spheres in motion: sphere k of trajectory b drifts with a constant seeded velocity
    (0.5 .. 1.5 radii over a quarter of the horizon) and is at its static centre -- on the reference path -- at the knot whose
    reference position is nearest to that centre, so the path violates it there; a velocity is halved until the sphere is
    clear of the reference positions of knots 0 and N.  Returns (prob, x0_q, x0_xi, us0, obstacles [B, N+1, K, 4]), the
    per-knot rows (cx, cy, cz, r) of set_al_obstacles."""
    prob, x0_q, x0_xi, us0, obs = se3_obstacle_field(B, K, N=N, seed=seed)
    rng = np.random.default_rng(seed + 4)
    t = prob.q_ref[:, :3, 3]
    s = np.arange(N + 1, dtype=np.float64)
    mov = np.empty((B, N + 1, K, 4))
    for b in range(B):
        for k in range(K):
            c, r = obs[b, k, :3], obs[b, k, 3]
            i0 = int(np.argmin(np.sum((t - c) ** 2, axis=1)))
            d = rng.normal(size=3)
            v = rng.uniform(0.5, 1.5) * r / max(1, N // 4) * d / np.linalg.norm(d)  # per knot
            while True:
                ck = c + (s - i0)[:, None] * v
                if all(np.sum((t[i] - ck[i]) ** 2) > r * r for i in (0, N)):
                    break
                v = 0.5 * v
            mov[b, :, k, :3], mov[b, :, k, 3] = ck, r
    return prob, x0_q, x0_xi, us0, mov


def se3_mpc_obstacles(B, steps, N=200, K=1, seed=SEED, **mpc_kw):
    """se3_mpc's inputs (mpc_kw: its T, R and sigmas) plus K keep-out spheres per trajectory on its own path, where the closed
    loop reaches them within `steps`: sphere k of trajectory b is placed by _obstacle_field's rule (radii 0.2 .. 0.4, moved by at
    most 0.3 r off the path) on the stretch of world knots t0[b] .. t0[b] + steps that the loop travels, so its knot lies in
    t0[b] + [steps // 4, 3 * steps // 4).  The drifting variant follows se3_moving_obstacle_field's rule in world time: a constant
    seeded velocity (0.5 .. 1.5 radii over a quarter of the horizon, N // 4 knots), the sphere at its static centre at the world knot of that stretch
    nearest to it, the velocity halved until the sphere is clear of the path at world knots t0[b] and t0[b] + steps.
    Returns (prob, x0_q, x0_xi, path_q, path_xi, t0, noise, obstacles [B, K, 4], obstacle_paths [B, T+1, K, 4]): the first
    seven are se3_mpc's, the last two what mpc(obstacles=) and mpc(obstacle_paths=) take."""
    prob, x0_q, x0_xi, path_q, path_xi, t0, noise = se3_mpc(B, steps, N=N, seed=seed, **mpc_kw)
    T = path_q.shape[1] - 1
    world = np.clip(t0[:, None].astype(np.int64) + np.arange(steps + 1)[None, :], 0, T)   # [B, steps+1]
    stretch = path_q[np.arange(B)[:, None], world]
    obs = _obstacle_field(stretch, B, K, 0.2, 0.4, seed + 3)
    rng = np.random.default_rng(seed + 6)
    s = np.arange(T + 1, dtype=np.float64)
    mov = np.empty((B, T + 1, K, 4))
    for b in range(B):
        t = stretch[b][:, :3, 3]
        for k in range(K):
            c, r = obs[b, k, :3], obs[b, k, 3]
            i0 = int(world[b, int(np.argmin(np.sum((t - c) ** 2, axis=1)))])
            d = rng.normal(size=3)
            v = rng.uniform(0.5, 1.5) * r / max(1, N // 4) * d / np.linalg.norm(d)  # per knot
            covered = any(np.sum((t[j] - c) ** 2) <= r * r for j in (0, steps))  # a stretch so short that no drift clears its ends
            while True:
                ck = c + (s - i0)[:, None] * v
                if covered or all(np.sum((t[j] - ck[world[b, j]]) ** 2) > r * r for j in (0, steps)):
                    break
                v = 0.5 * v
            mov[b, :, k, :3], mov[b, :, k, 3] = ck, r
    return prob, x0_q, x0_xi, path_q, path_xi, t0, noise, obs, mov


def se3_mpc_inspection(B, steps, N=200, seed=SEED, **mpc_kw):
    """se3_mpc's inputs (mpc_kw: its T, R and sigmas) under se3_inspection's two pose slots per trajectory (kinds
    INSPECTION_KINDS), stated in world time over the stretch of world knots t0[b] .. t0[b] + steps that the loop travels:
      a tilt cone about world z, (0, 0, 1, c_s): behind a ramp-in of r = max(2, steps // 4) knots, c lies 0.2 above the smallest
               n^T R e3 of trajectory b's path on the rest of the stretch (and at most 0.9; half-way from that smallest value
               to 1 where the stretch is more upright than 0.9 throughout), so the path's most tilted knot there leaves the
               cone, by up to 0.2.  A path moved by a rigid motion may be at its most tilted right where the loop
               starts, so at world knot t0[b] (and before it) the cosine lies 0.1 below the smaller of the start's own n^T R e3
               and the path's there (half-way to -1 where that is nearer), never above c, and rises to c linearly over the
               ramp-in: the start is inside;
      a view cone on a target that drifts along a world-time line, (p_s, c): p_s moves from 3 ahead of trajectory b's own start
               pose (along its forward axis: on the cone's axis at the start) at world knot t0[b] to 3 ahead of the path's last
               pose at world knot T, as se3_inspection's target runs to the end of its horizon -- every window of the loop looks
               N knots ahead, and a target that stopped at the end of the stretch would be run over by the path behind it, where
               the view row has no gradient -- and rests before t0[b]; the distance ahead, 3, grows by half until the target
               keeps 1 away from the path at every world knot from t0[b] on; c lies a fifth of the way from the smallest e1^T b / |b|
               of the second half of the stretch under that target to 1.
    The reference path leaves both cones on the stretch in every trajectory; the start of every trajectory satisfies both at its
    world knot.  Both are checkable with pose_margin (tests/test_pose_mpc_cpu.py).  Returns (prob, x0_q, x0_xi, path_q, path_xi, t0, noise, pose_paths [B, T+1, 2, 4], kinds): the
    first seven are se3_mpc's, the last two what mpc(pose_paths=, pose_kinds=) takes."""
    prob, x0_q, x0_xi, path_q, path_xi, t0, noise = se3_mpc(B, steps, N=N, seed=seed, **mpc_kw)
    T = path_q.shape[1] - 1
    slots = np.empty((B, T + 1, 2, 4))
    s = np.arange(T + 1, dtype=np.float64)
    ramp = max(2, steps // 4)
    for b in range(B):
        R, t, X0 = path_q[b, :, :3, :3], path_q[b, :, :3, 3], np.asarray(x0_q[b]).reshape(4, 4)
        a, e = int(t0[b]), min(int(t0[b]) + steps, T)
        if e - a <= ramp:
            raise ValueError("se3_mpc_inspection: trajectory %d travels %d knots, the ramp-in alone takes %d" % (b, e - a, ramp))
        m = R[:, 2, 2]
        lo = m[a + ramp: e + 1].min()
        c = min(lo + 0.2, max(0.9, 0.5 * (lo + 1.0)))
        m_in = min(X0[2, 2], m[a])
        c_in = min(c, m_in - min(0.1, 0.5 * (m_in + 1.0)))
        slots[b, :, 0, :3] = (0.0, 0.0, 1.0)
        slots[b, :, 0, 3] = c_in + np.clip((s - a) / ramp, 0.0, 1.0) * (c - c_in)
        ahead = 3.0
        while True:
            p0, p1 = X0[:3, 3] + ahead * X0[:3, 0], t[T] + ahead * R[T][:, 0]
            p = p0 + np.clip((s - a) / (T - a), 0.0, 1.0)[:, None] * (p1 - p0)
            if np.linalg.norm(p[a:] - t[a:], axis=1).min() >= 1.0:
                break
            ahead *= 1.5
        bv = np.einsum("iac,ia->ic", R, p - t)
        cv = bv[:, 0] / np.linalg.norm(bv, axis=1)
        late = cv[(a + e + 1) // 2: e + 1].min()
        slots[b, :, 1, :3], slots[b, :, 1, 3] = p, late + 0.2 * (1.0 - late)
    return prob, x0_q, x0_xi, path_q, path_xi, t0, noise, slots, INSPECTION_KINDS


def se3_crossing_fleet(F, G, N=40, separation=0.3, seed=SEED):
    """F fleets of G members whose paths cross: member p tracks g_p q_ref, with g_p the rotation by p pi / G about world z
    through the reference's position at knot N // 2 plus a z shift of 0.3 separation p -- every pair of paths passes within
    less than `separation` near the middle knot.  xi_ref is shared (body twists do not change under a left multiplication);
    member (f, p) starts at g_p applied to fleet f's perturbed start of se3_tracking(F, N, R_scale=1e-3).  Batch index
    f * G + p.  Returns (prob, x0_q, x0_xi, us0, q_ref [F G, N+1, 4, 4], xi_ref [F G, N+1, 6])."""
    prob, q, xi, _ = se3_tracking(F, N=N, R_scale=1e-3, seed=seed)
    c = prob.q_ref[N // 2][:3, 3]
    B = F * G
    x0_q, x0_xi = np.empty((B, 4, 4)), np.empty((B, 6))
    q_ref, xi_ref = np.empty((B, N + 1, 4, 4)), np.empty((B, N + 1, 6))
    for p in range(G):
        g = np.eye(4)
        g[:3, :3] = _so3_exp(np.array([0.0, 0.0, p * np.pi / G]))
        g[:3, 3] = c - g[:3, :3] @ c + np.array([0.0, 0.0, 0.3 * separation * p])
        for f in range(F):
            b = f * G + p
            x0_q[b], x0_xi[b] = g @ q[f], xi[f]
            q_ref[b], xi_ref[b] = g @ prob.q_ref, prob.xi_ref
    return prob, x0_q, x0_xi, np.zeros((B, N, 6)), q_ref, xi_ref
