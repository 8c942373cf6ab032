"""The pose constraints of tolg_set_al_pose_constraints restated in NumPy, for tests/test_pose_constraints_cpu.py and
tests/test_gpu_pose_constraints.py: per-kind row, gradient and margin, the augmented-Lagrangian terms they add to the
linearisation, the multiplier rule, and seeded slots with knots on both sides of every surface.  Slot k has fields (f0, f1, f2,
c); body axes e3 = (0, 0, 1) and e1 = (1, 0, 0); error coordinates X Exp(delta), twist order [omega, v]:
  0 tilt cone  n = (f0, f1, f2), |n| = 1   g = c - n^T R e3                    g_omega = (R^T n) x e3   g_v = 0               margin n^T R e3 - c
  1 view cone  p = (f0, f1, f2)            g = c |b| - e1^T b, b = R^T (p - t)   g_omega = b x e1         g_v = e1 - c b / |b|   margin e1^T b / |b| - c"""
import numpy as np

TILT, VIEW = 0, 1
NAMES = ("tilt_cone", "view_cone")
E1, E3 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
MIXED = (VIEW, TILT, TILT, VIEW)   # K = 4, each kind twice


def rows(xs_q, geo, kinds):
    """xs_q [..., 4, 4] poses, geo [..., K, 4] slots (leading shapes that broadcast), kinds [K].  Returns (g [..., K], g_x
    [..., K, 6] = [g_omega, g_v], margin [..., K]), each kind by its own formula."""
    xs_q, geo = np.asarray(xs_q, float), np.asarray(geo, float)
    R, t = xs_q[..., :3, :3], xs_q[..., :3, 3]
    g, gx, mg = [], [], []
    for k, kd in enumerate(kinds):
        f = geo[..., k, :]
        c = f[..., 3]
        if kd == TILT:
            a = np.einsum("...ac,...a->...c", R, np.broadcast_to(f[..., :3], np.broadcast_shapes(f[..., :3].shape, t.shape)))
            g.append(c - a[..., 2])
            gx.append(np.concatenate([np.cross(a, E3), np.zeros_like(a)], axis=-1))
            mg.append(a[..., 2] - c)
            continue
        b = np.einsum("...ac,...a->...c", R, f[..., :3] - t)
        nb = np.linalg.norm(b, axis=-1)
        g.append(c * nb - b[..., 0])
        gx.append(np.concatenate([np.cross(b, E1), E1 - (c / nb)[..., None] * b], axis=-1))
        mg.append(b[..., 0] / nb - c)
    return np.stack(g, -1), np.stack(gx, -2), np.stack(mg, -1)


def per_knot(slots):
    """slots [B, K, 4] or [B, N+1, K, 4] as [B, 1 or N+1, K, 4]"""
    slots = np.asarray(slots, float)
    return slots[:, None] if slots.ndim == 3 else slots


def g_rows(xs_q, slots, kinds):
    """The rows of every knot: [B, N+1, K] of xs_q [B, N+1, 4, 4]"""
    return rows(xs_q, per_knot(slots), kinds)[0]


def terms(xs_q, slots, kinds, lam, imu):
    """Per (b, i) the l, l_x[0:6] and l_xx[0:6, 0:6] the slots add, and g: ALConstrainedCost's Gauss-Newton terms."""
    g, gx, _ = rows(xs_q, per_knot(slots), kinds)                     # [B, N+1, K], [B, N+1, K, 6]
    l = np.sum(lam * g + 0.5 * imu * g * g, axis=-1)
    lx = np.einsum("bikc,bik->bic", gx, lam + imu * g)
    lxx = np.einsum("bik,bika,bikc->biac", imu, gx, gx)
    return g, l, lx, lxx


def se3_exp(d):
    """Exp of a twist [omega, v] as a 4x4 pose"""
    w, v = np.asarray(d[:3], float), np.asarray(d[3:], float)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        R, V = np.eye(3) + W + 0.5 * W @ W, np.eye(3) + 0.5 * W
    else:
        R = np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W
    X = np.eye(4)
    X[:3, :3], X[:3, 3] = R, V @ v
    return X


def random_poses(rng, shape, spread=2.0):
    """Poses with rotations all over SO(3) and positions within `spread`"""
    out = np.empty(tuple(shape) + (4, 4))
    for idx in np.ndindex(*shape):
        out[idx] = se3_exp(np.r_[rng.normal(size=3) * 1.5, rng.uniform(-spread, spread, 3)])
    return out


def mixed_slots(xs_q, kinds, seed, per_knot_form=False):
    """Slots of the given kinds about poses xs_q [B, N+1, 4, 4], so that every slot has knots on both sides of its surface: a
    tilt cone has a seeded unit axis and its cosine between the extremes of n^T R e3 over the knots; a view cone has a seeded
    target 2 .. 4 away from the path's middle and its cosine between the extremes of e1^T b / |b|.  Returns [B, K, 4], or
    with per_knot_form [B, N+1, K, 4]: the targets drifting by a seeded velocity and the cosines of the tilt cones by a seeded
    rate, re-centred per knot so that both signs stay."""
    rng = np.random.default_rng(seed)
    xs_q = np.asarray(xs_q, float)
    B, N1, K = xs_q.shape[0], xs_q.shape[1], len(kinds)
    out = np.empty((B, N1, K, 4))
    s = np.arange(N1)[:, None] / max(1, N1 - 1)
    for b in range(B):
        R, t = xs_q[b, :, :3, :3], xs_q[b, :, :3, 3]
        for k, kd in enumerate(kinds):
            if kd == TILT:
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                out[b, :, k, :3] = n
                m = R[:, :, 2] @ n
            else:
                d = rng.normal(size=3)
                p = t[N1 // 2] + rng.uniform(2.0, 4.0) * d / np.linalg.norm(d)
                p = p[None] + (s * rng.normal(size=3) * 0.5 if per_knot_form else 0.0)
                out[b, :, k, :3] = p
                bv = np.einsum("iac,ia->ic", R, p - t)
                m = bv[:, 0] / np.linalg.norm(bv, axis=1)
            c = m.min() + rng.uniform(0.3, 0.7) * (m.max() - m.min())
            out[b, :, k, 3] = c + (0.1 * (m.max() - m.min()) * (s[:, 0] - 0.5) if per_knot_form else 0.0)
    return out if per_knot_form else out[:, 0].copy()
