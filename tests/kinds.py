"""The position constraints of tolg_set_al_obstacle_kinds restated in NumPy, for tests/test_obstacle_kinds_cpu.py and
tests/test_gpu_obstacle_kinds.py: per-kind row, gradient and clearance, the augmented-Lagrangian terms they add to the
linearisation (test_gpu_obstacles._terms, generalised), the multiplier rule, and inputs that put every kind on both sides of its
surface.  Slot k has fields (f0, f1, f2, f3); with d = t - (f0, f1, f2):
  0 keep-out sphere  g = r^2 - |d|^2          grad_t g = -2 d            clearance |d| - r
  1 keep-in sphere   g = |d|^2 - r^2          grad_t g = 2 d             clearance r - |d|
  2 half-space       g = n.t - o              grad_t g = n               clearance o - n.t
  3 vertical column  g = r^2 - (dx^2 + dy^2)  grad_t g = -2 (dx, dy, 0)  clearance sqrt(dx^2 + dy^2) - r"""
import numpy as np

SPHERE, KEEP_IN, HALF_SPACE, COLUMN = 0, 1, 2, 3
NAMES = ("sphere", "keep_in", "half_space", "column")
CORRIDOR = (HALF_SPACE, HALF_SPACE, KEEP_IN, COLUMN, COLUMN, SPHERE)  # workloads.CORRIDOR_KINDS by number


def rows(t, geo, kinds):
    """t [..., 3] positions, geo [..., K, 4] slots (leading shapes that broadcast), kinds [K].  Returns (g [..., K], grad_t g
    [..., K, 3], clearance [..., K]), each kind by its own formula."""
    t, geo = np.asarray(t, float), np.asarray(geo, float)
    g, grad, clear = [], [], []
    for k, kd in enumerate(kinds):
        f = geo[..., k, :]
        if kd == HALF_SPACE:
            n = np.broadcast_to(f[..., :3], np.broadcast_shapes(f[..., :3].shape, t.shape))
            nt = np.sum(n * t, axis=-1)
            g.append(nt - f[..., 3]); grad.append(n + 0.0); clear.append(f[..., 3] - nt)
            continue
        d = t - f[..., :3]
        if kd == COLUMN:
            d = d * np.array([1.0, 1.0, 0.0])
        d2, r = np.sum(d * d, axis=-1), f[..., 3]
        if kd == KEEP_IN:
            g.append(d2 - r ** 2); grad.append(2.0 * d); clear.append(r - np.sqrt(d2))
        else:
            g.append(r ** 2 - d2); grad.append(-2.0 * d); clear.append(np.sqrt(d2) - r)
    return np.stack(g, -1), np.stack(grad, -2), np.stack(clear, -1)


def per_knot(obs):
    """obs [B, K, 4] or [B, N+1, K, 4] as [B, 1 or N+1, K, 4]"""
    obs = np.asarray(obs, float)
    return obs[:, None] if obs.ndim == 3 else obs


def g_rows(xs_q, obs, kinds):
    """The rows of every knot: [B, N+1, K] of xs_q [B, N+1, 4, 4]"""
    return rows(xs_q[..., :3, 3], per_knot(obs), kinds)[0]


def g_x(X, geo, kinds):
    """g_x of one pose X [4, 4] in the error coordinates of X Exp(delta), twist order [omega, v]: [K, 12] = [0, (grad_t g)^T
    R, 0]"""
    out = np.zeros((len(kinds), 12))
    out[:, 3:6] = rows(X[:3, 3], geo, kinds)[1] @ X[:3, :3]
    return out


def terms(xs_q, obs, kinds, lam, imu):
    """Per (b, i) the l, l_x[3:6] and l_xx[3:6, 3:6] the slots add, and g: test_gpu_obstacles._terms with the row and the
    gradient of every slot's kind, gv = R^T grad_t g."""
    R, t = xs_q[..., :3, :3], xs_q[..., :3, 3]
    g, grad, _ = rows(t, per_knot(obs), kinds)                       # [B, N+1, K], [B, N+1, K, 3]
    gv = np.einsum("biac,bika->bikc", R, grad)
    l = np.sum(lam * g + 0.5 * imu * g * g, axis=-1)
    lx = np.einsum("bikc,bik->bic", gv, lam + imu * g)
    lxx = np.einsum("bik,bika,bikc->biac", imu, gv, gv)
    return g, l, lx, lxx


def update(g, lam, imu, mu, mu_scale=10.0):
    """The multiplier rule on rows g (the same for every kind): tests.checks.update_restated"""
    from tests.checks import update_restated
    return update_restated(g, lam, imu, mu, mu_scale)


def clearance_of(t, slots, kinds):
    """tests.limits.clearance_of with the clearance of every slot's kind: t [N+1, 3], slots [K, 4] or [N+1, K, 4].  Returns
    (the minimum over knots and slots, the first knot that attains it under a strict < with knots and slots ascending, the
    smallest of the other knots' own minima)."""
    sl = np.asarray(slots, float)
    c = rows(np.asarray(t, float), sl[None] if sl.ndim == 2 else sl, kinds)[2]   # [N+1, K]
    best, knot = np.inf, 0
    for i in range(c.shape[0]):
        for k in range(c.shape[1]):
            if c[i, k] < best:
                best, knot = c[i, k], i
    others = np.delete(np.fmin.reduce(c, axis=1), knot)
    return best, knot, (others.min() if others.size else np.inf)


def mixed_slots(t, kinds, seed, moving=False):
    """Slots of the given kinds about positions t [B, N+1, 3], so that every slot has knots on both sides of its surface: a
    sphere, geofence or column is centred near a knot of the path, or away from it, with a radius between the smallest and
    the largest distance of the knots from its centre (axis); a half-space has a seeded unit normal and its offset between
    the extremes of n.t.  Returns obs [B, K, 4], or with moving [B, N+1, K, 4]: the same slots drifting by a seeded velocity."""
    rng = np.random.default_rng(seed)
    B, N1, K = t.shape[0], t.shape[1], len(kinds)
    obs = np.empty((B, K, 4))
    for b in range(B):
        for k, kd in enumerate(kinds):
            if kd == HALF_SPACE:
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                s = t[b] @ n
                obs[b, k] = (*n, s.min() + rng.uniform(0.3, 0.7) * (s.max() - s.min()))
                continue
            c = t[b, rng.integers(N1)] + rng.normal(size=3) * 0.3 * np.ptp(t[b], axis=0).max()
            d = t[b] - c
            dist = np.linalg.norm(d[:, :2] if kd == COLUMN else d, axis=1)
            obs[b, k] = (*c, dist.min() + rng.uniform(0.3, 0.7) * (dist.max() - dist.min()))
    if not moving:
        return obs
    scale = 0.02 * np.ptp(t, axis=1).max()
    vel = rng.normal(size=(B, 1, K, 4)) * scale / N1
    vel[..., 3] = 0.0
    vel[:, :, [k for k, kd in enumerate(kinds) if kd == HALF_SPACE]] = 0.0   # a drifting normal would leave the unit sphere
    return obs[:, None] + vel * np.arange(N1)[None, :, None, None]
