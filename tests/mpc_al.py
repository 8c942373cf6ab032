"""The outer update of a constrained MPC step (tolg_al_mpc_step) restated in NumPy, for tests/test_mpc_constrained_cpu.py and
tests/test_gpu_mpc_constrained.py: the rows, the rule and the shift by indexing."""
import numpy as np


def g_box(us, lb, ub):
    """The box rows [lb - u_i; u_i - ub]: [B, N, 2m] of us [B, N, m]"""
    return np.concatenate([lb - us, us - ub], axis=-1)


def g_spheres(xs_q, obs):
    """The sphere rows r^2 - |t_i - c_ik|^2: [B, N+1, K] of xs_q [B, N+1, 4, 4] and obs [B, K, 4] or [B, N+1, K, 4]"""
    if obs.ndim == 3:
        obs = obs[:, None]
    d = xs_q[..., :3, 3][:, :, None, :] - obs[..., :3]
    return obs[..., 3] ** 2 - np.sum(d * d, axis=-1)


def shifted(a):
    """Row i takes row i+1, the last row is held: a [B, rows, ...]"""
    rows = a.shape[1]
    return a[:, np.minimum(np.arange(rows) + 1, rows - 1)]


def al_mpc_step_restated(mu, mu_scale, mu_max, tol_constr, shift, box=None, spheres=None):
    """box, spheres: (g, lam, imu) of the rows attached, or None.  Returns (maxviol [B], mu_new [B], box', spheres') with
    box' / spheres' = (lam', imu') or None."""
    B = mu.shape[0]
    mv = np.zeros(B) if box is not None else np.full(B, -np.inf)
    for rows in (box, spheres):
        if rows is not None:
            mv = np.fmax(mv, np.fmax.reduce(rows[0].reshape(B, -1), axis=1))
    mu_new = np.where(mv < tol_constr, mu, np.minimum(mu_scale * mu, mu_max))
    out = []
    for rows in (box, spheres):
        if rows is None:
            out.append(None)
            continue
        g, lam, imu = rows
        ln = np.maximum(0.0, lam + imu * g)
        im = np.where((g < 0) & (ln == 0), 0.0, mu_new[:, None, None])
        out.append((shifted(ln), shifted(im)) if shift else (ln, im))
    return mv, mu_new, out[0], out[1]
