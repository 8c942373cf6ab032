"""Pose slots in the receding-horizon step (tolg_al_mpc_step_pose: tolg_al_mpc_step with a third row set), for
tests/test_pose_mpc_cpu.py and tests/test_gpu_pose_mpc.py: tests/mpc_al.py's restatement extended to a third (g, lam, imu) set, and seeded inputs of the step
in NumPy alone, so that what the GPU test asserts about them on the CPU can be checked without a GPU."""
import numpy as np

from tests import pose_kinds as pk
from tests.mpc_al import g_box, g_spheres, shifted
from tests.test_gpu_mpc_constrained import _step_inputs  # (NumPy alone: the box, the positions and the spheres of its step test)

TILE = 512             # AL_STEP_TILE (csrc/tolg_kernels.hip)
N_LONG = 2 * TILE + 2  # Kp = 1: N + 1 pose rows = two tiles plus three rows
CASES = ("pose", "pose_knot", "box+pose", "static+pose", "box+moving+pose_knot")
CLEAR = 1e-9           # every restated |g| and every nonzero |lambda + I_mu g| lies further than this from its branch point
U = 2.0 ** -53         # the unit roundoff of a double
# The largest I_mu of the seeded pose multipliers.  lambda' = lambda + I_mu g is compared at rtol 1e-12 with a floor of 1e-15, and
# the sum cancels: what the kernel's row and NumPy's differ by reaches lambda' times I_mu whatever lambda' is.  The two rows are
# the same formula rounded in another order (fused multiply-adds, the order of a dot product), and differ by at most
# POSE_ROW_ULPS U D with D = |p - t| for a view cone and 1 for a tilt cone (lambda_error_bound has the count); with targets 2 .. 4
# from the path, 20 for a satisfied trajectory, and positions a few units apart D stays below 30, so I_mu <= 0.01 keeps the
# difference below the floor on every row -- test_step_against_the_restatement asserts that row by row before it compares.  (At I_mu up to 20, the spheres' range,
# whose rows are 20 times smaller, one row in 10^5 lands where the sum cancels to 10^-4 and misses the floor by a tenth.)
POSE_IMU = 0.01
POSE_ROW_ULPS = 28


def al_mpc_step_restated3(mu, mu_scale, mu_max, tol_constr, shift, box=None, spheres=None, pose=None):
    """tests/mpc_al.al_mpc_step_restated with the pose rows as a third set: box, spheres, pose = (g, lam, imu) of the rows
    attached, or None.  One mu per problem and a joint maxviol; the pose multipliers [B, N+1, Kp] shift as the spheres' do.
    Returns (maxviol [B], mu_new [B], box', spheres', pose') with each ' = (lam', imu') or None."""
    B = mu.shape[0]
    sets = (box, spheres, pose)
    mv = np.zeros(B) if box is not None else np.full(B, -np.inf)
    for rows in sets:
        if rows is not None:
            mv = np.fmax(mv, np.fmax.reduce(rows[0].reshape(B, -1), axis=1))
    mu_new = np.where(mv < tol_constr, mu, np.minimum(mu_scale * mu, mu_max))
    out = []
    for rows in sets:
        if rows is None:
            out.append(None)
            continue
        g, lam, imu = rows
        ln = np.maximum(0.0, lam + imu * g)
        im = np.where((g < 0) & (ln == 0), 0.0, mu_new[:, None, None])
        out.append((shifted(ln), shifted(im)) if shift else (ln, im))
    return (mv, mu_new) + tuple(out)


def rotations(rng, shape):
    """Rotations all over SO(3), [..., 3, 3]: Rodrigues on seeded rotation vectors, angles up to about pi"""
    w = rng.normal(size=tuple(shape) + (3,)) * 1.2
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    W = np.zeros(tuple(shape) + (3, 3))
    W[..., 0, 1], W[..., 0, 2], W[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    W[..., 1, 2], W[..., 2, 0], W[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)


def pose_kinds_of(Kp, seed):
    """Kp kinds, both of them from Kp = 2 on, the first one alternating with the seed (Kp = 1 runs either kind)"""
    return tuple(int(k) for k in np.roll(np.array(pk.MIXED * 2), seed)[:Kp])


def mults(rng, B, rows, W, imu=20.0):
    """Random multipliers (lam up to 1, I_mu up to `imu`) with some I_mu = 0 and some lambda = 0: [B, rows, W] each"""
    return [rng.uniform(0.0, hi, (B, rows, W)) * (rng.uniform(size=(B, rows, W)) > 0.3) for hi in (1.0, imu)]


def step_case(N, m, B, Ks, Kp, case, sat, seed):
    """The inputs of one tolg_al_mpc_step_pose under `case` (one of CASES: which row sets are attached, and in which geometry
    form) in NumPy.  Poses: the positions of test_gpu_mpc_constrained's _step_inputs under seeded rotations; pose slots:
    pose_kinds.mixed_slots about them, so that every slot has knots on both sides of its surface; the trajectories `sat` satisfy
    everything -- upright (R = 1), under a tilt cone about z of cosine 0.5 and view cones of cosine 0.5 on a target 20 ahead of
    their middle, in the box, 1000 from the spheres.  Ks spheres, Kp pose slots.
    Returns a dict: lb, ub, us, xs_q, obs, slots, kinds, and box / sph / pose = [lam, imu] or None."""
    rng = np.random.default_rng(1000 + seed)
    lb, ub, us, xs_q, obs = _step_inputs(N, m, B, Ks, "moving" in case, sat, seed)
    pos = xs_q[..., :3, 3].copy()
    xs_q[..., :3, :3] = rotations(rng, (B, N + 1))
    for b in sat:
        xs_q[b, :, :3, :3] = np.eye(3)
    kinds = pose_kinds_of(Kp, seed)
    per_knot = "pose_knot" in case
    slots = pk.mixed_slots(xs_q, kinds, seed, per_knot)
    for b in sat:
        for k, kd in enumerate(kinds):
            far = (0.0, 0.0, 1.0, 0.5) if kd == pk.TILT else tuple(pos[b].mean(axis=0) + (20.0, 0.0, 0.0)) + (0.5,)
            slots[b, ..., k, :] = far
    return dict(lb=lb, ub=ub, us=us, xs_q=xs_q, obs=obs, slots=slots, kinds=kinds,
                box=mults(rng, B, N, 2 * m) if "box" in case else None,
                sph=mults(rng, B, N + 1, Ks) if "static" in case or "moving" in case else None,
                pose=mults(rng, B, N + 1, Kp, POSE_IMU))


def step_rows(c):
    """The (g, lam, imu) sets of a step_case: box, spheres, pose"""
    return [None if c["box"] is None else (g_box(c["us"], c["lb"], c["ub"]), *c["box"]),
            None if c["sph"] is None else (g_spheres(c["xs_q"], c["obs"]), *c["sph"]),
            (pk.g_rows(c["xs_q"], c["slots"], c["kinds"]), *c["pose"])]


def clear_of_branch_points(rows):
    """The smallest |g| and the smallest nonzero |lambda + I_mu g| over every row of every set: I_mu' is a discrete choice on
    the signs of both, so a restatement and a kernel that round a row differently may disagree where either is within rounding
    of zero."""
    lo = np.inf
    for r in rows:
        if r is not None:
            g, lam, imu = r
            v = np.abs(lam + imu * g)
            lo = min(lo, np.abs(g).min(), v[v != 0].min() if (v != 0).any() else np.inf)
    return lo


def lambda_error_bound(c, rows):
    """The largest ratio, over the pose rows with lambda' > 0, of a bound on |lambda'_kernel - lambda'_NumPy| to what the
    comparison allows, 1e-15 + 1e-12 lambda'.  The bound: both sides form d = p - t alike; b = R^T d is three products summed, each
    side within 3 U D of the exact one; |b| adds the square root and the sum of squares, 7.7 U D in all; c |b| - b_0 and its last
    rounding bring a side to 14 U D, so two sides differ by at most POSE_ROW_ULPS U D (a tilt row, c - n^T R e3 with |n| = 1:
    D = 1).  lambda + I_mu g then adds U I_mu |g| for NumPy's rounded product, which the kernel fuses, and 2 U lambda' for the
    final roundings."""
    g, lam, imu = rows[2]
    xs_q, slots = c["xs_q"], pk.per_knot(c["slots"])
    D = np.ones(g.shape)
    for k, kd in enumerate(c["kinds"]):
        if kd == pk.VIEW:
            D[..., k] = np.linalg.norm(slots[..., k, :3] - xs_q[..., :3, 3], axis=-1)
    ln = np.maximum(0.0, lam + imu * g)
    bound = imu * (POSE_ROW_ULPS * D + np.abs(g)) * U + 2 * U * ln
    on = ln > 0
    return (bound[on] / (1e-15 + 1e-12 * ln[on])).max() if on.any() else 0.0


def step_grid(N):
    """(B, Kp, case, sat, seed) of test_step_against_the_restatement at horizon N: B in 1, 5, 13 (padded lanes; the satisfied
    trajectory last), Kp in 1, 3, 8 (3: the 16- and the 8-byte paths of the paired loads both run), every case"""
    seed = 0
    for B in (1, 5, 13):
        for Kp in (1, 3, 8):
            for case in CASES:
                for sat in ([[], [0]] if B == 1 else [[B - 1]]):
                    seed += 1
                    yield B, Kp, case, sat, 23 * N + seed
