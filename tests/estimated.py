"""Output feedback (tolg_policy_covariance_estimated, tolg_policy_rollout_estimated): the host restatements of the two
recursions of include/tolg.h, statement for statement, from oracle primitives, and the inputs the CPU and GPU tests share.
A plain module (pytest does not collect it)."""
import numpy as np

from oracle import bridge as ob
from tests.support import (KW, assert_coverage, determined, embed, estimated_need, estimated_site_tags, nudged, op_of, psd,
                           sample_spread)

SO3_COORDS = [0, 1, 2, 6, 7, 8]
MC_SIGMA = (1e-3, 1e-3, 2e-4)  # pose, twist, noise: the scales of tests/test_covariance_cpu.py's sampled check
MC_MULT = 5.0                  # ... and its bound, in standard errors of a Gaussian sample covariance


def measured(mask):
    return [j for j in range(12) if (mask >> j) & 1]


def _sym(a, n, T):
    return np.zeros((n, n), dtype=T) if a is None else 0.5 * (np.asarray(a, T) + np.asarray(a, T).T)


def restate_covariance_estimated(op, q_nom, xi_nom, u_nom, K, mask, V, Sigma0=None, W=None, dtype=np.float64):
    """The recursion of tolg_policy_covariance_estimated from ob.fx_fu only, carried in `dtype` (np.longdouble: the reference of
    the conditioning test; the Jacobians are the oracle's doubles either way).
    q_nom [N+1, 4, 4], xi_nom [N+1, 6], u_nom [N, m], K [N, m, 12], mask int, V [12] (read on measured coordinates only),
    Sigma0 [12, 12], W [6, 6] (None: zero).  Returns a dict: Sigma, P_prior, P_post, L [N+1, 12, 12], var_x, var_est [N+1, 12],
    var_u [N, m], pos_cov [N+1, 3, 3]."""
    T = dtype
    N, m = u_nom.shape
    meas = measured(mask)
    P, Sh = _sym(Sigma0, 12, T), np.zeros((12, 12), dtype=T)
    EW = np.zeros((12, 12), dtype=T)
    EW[6:, 6:] = _sym(W, 6, T)
    Vt = None if V is None else np.asarray(V, T)
    out = {k: np.zeros((N + 1, 12, 12), dtype=T) for k in ("Sigma", "P_prior", "P_post", "L")}
    var_u = np.zeros((N, m), dtype=T)
    for i in range(N + 1):
        out["Sigma"][i] = Sh + P
        out["P_prior"][i] = Pm = P.copy()
        for j in meas:
            s = P[j, j] + Vt[j]
            c = P[:, j].copy()
            P = P - np.outer(c, c) / s
        out["P_post"][i] = P
        for j in meas:
            out["L"][i][:, j] = P[:, j] / Vt[j]
        Sh = Sh + (Pm - P)
        if i == N:
            break
        Fx, Fu = ob.fx_fu(op, q_nom[i], xi_nom[i], u_nom[i])
        A, Ki = np.asarray(Fx, T), np.asarray(K[i], T)
        Acl = A + np.asarray(Fu, T) @ Ki
        var_u[i] = np.einsum("uc,cd,ud->u", Ki, Sh, Ki)
        P = A @ P @ A.T + EW
        P = 0.5 * (P + P.T)
        Sh = Acl @ Sh @ Acl.T
        Sh = 0.5 * (Sh + Sh.T)
    out["var_x"] = np.einsum("icc->ic", out["Sigma"]).copy()
    out["var_est"] = np.einsum("icc->ic", out["P_post"]).copy()
    out["var_u"] = var_u
    R = np.asarray(q_nom, T).reshape(N + 1, 4, 4)[:, :3, :3]
    out["pos_cov"] = np.einsum("iap,ipq,ibq->iab", R, out["Sigma"][:, 3:6, 3:6], R)
    return out


def restate_rollout_estimated(op, q_nom, xi_nom, u_nom, K, L, mask, dx0=None, w=None, n=None, S=1):
    """S samples of tolg_policy_rollout_estimated's loop for one trajectory from oracle primitives only (ob.f, ob.rminus,
    ob.se3_exp, ob.cost).  L [N+1, 12, 12], dx0 [S, 12], w [S, N, 6], n [S, N+1, 12] (None: zero).
    Returns J [S], xs_q [S, N+1, 4, 4], xs_xi [S, N+1, 6], us [S, N, m], est_q [S, N+1, 4, 4], est_xi [S, N+1, 6]."""
    N, m = u_nom.shape
    keep = np.zeros(12)
    keep[measured(mask)] = 1.0
    J = np.zeros(S)
    xs_q = np.zeros((S, N + 1, 4, 4)); xs_xi = np.zeros((S, N + 1, 6)); us = np.zeros((S, N, m))
    est_q = np.zeros((S, N + 1, 4, 4)); est_xi = np.zeros((S, N + 1, 6))
    for s in range(S):
        q, xi = np.array(q_nom[0], float).reshape(4, 4), np.array(xi_nom[0], float)
        qh, xih = q.copy(), xi.copy()
        if dx0 is not None:
            q = q @ ob.se3_exp(dx0[s, :6])
            xi = xi + dx0[s, 6:]
        for i in range(N + 1):
            qy, xiy = (q, xi) if n is None else (q @ ob.se3_exp(n[s, i, :6]), xi + n[s, i, 6:])
            r = np.r_[ob.rminus(qy, qh), xiy - xih] * keep
            d = L[i] @ r
            qh, xih = qh @ ob.se3_exp(d[:6]), xih + d[6:]
            xs_q[s, i], xs_xi[s, i], est_q[s, i], est_xi[s, i] = q, xi, qh, xih
            if i == N:
                break
            eh = np.r_[ob.rminus(qh, q_nom[i]), xih - xi_nom[i]]
            u = u_nom[i] + K[i] @ eh
            us[s, i] = u
            J[s] += ob.cost(op, q, xi, u, i)[0]
            q, xi = ob.f(op, q, xi, u)
            if w is not None:
                xi = xi + w[s, i]
            qh, xih = ob.f(op, qh, xih, u)
        J[s] += ob.cost(op, q, xi, None, N, terminal=True)[0]
    return J, xs_q, xs_xi, us, est_q, est_xi


def errors_of(q_nom, xi_nom, xs_q, xs_xi):
    """e_i = [Log(q*_i^-1 q_i); xi_i - xi*_i] of S trajectories: [S, N+1, 12]."""
    S, N1 = xs_xi.shape[:2]
    e = np.zeros((S, N1, 12))
    for s in range(S):
        for i in range(N1):
            e[s, i, :6] = ob.rminus(np.asarray(xs_q[s, i]).reshape(4, 4), q_nom[i])
            e[s, i, 6:] = xs_xi[s, i] - xi_nom[i]
    return e


def errors_batch(q_nom, xi_nom, xs_q, xs_xi):
    """errors_of in numpy, for the sample counts of the device tests: Log of E = q*_i^-1 q_i as [w; Jl(w)^-1 t] with
    w = (theta / sin theta) vee(R - R^T) / 2, series below 1e-4 rad; for deviations well inside pi / 2 (it takes theta from
    atan2(|vee|, (tr R - 1) / 2) and does not treat the band at pi).  tests/test_estimated_cpu.py holds it to errors_of."""
    q_nom = np.asarray(q_nom, float).reshape(-1, 4, 4)
    X = np.asarray(xs_q, float).reshape(xs_xi.shape[0], -1, 4, 4)
    Rn, tn = q_nom[:, :3, :3], q_nom[:, :3, 3]
    R = np.einsum("ipa,sipb->siab", Rn, X[:, :, :3, :3])
    t = np.einsum("ipa,sip->sia", Rn, X[:, :, :3, 3] - tn[None])
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    sn = np.linalg.norm(v, axis=-1)
    cs = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    th = np.arctan2(sn, cs)
    small = th < 1e-4
    ths = np.where(small, 1.0, th)
    w = v * np.where(small, 1.0 + th * th / 6.0, ths / np.where(small, 1.0, sn))[..., None]
    c = np.where(small, 1.0 / 12.0 + th * th / 720.0, 1.0 / ths ** 2 - (1.0 + cs) / (2.0 * ths * np.where(small, 1.0, sn)))
    wt = np.cross(w, t)
    rho = t - 0.5 * wt + c[..., None] * np.cross(w, wt)
    return np.concatenate([w, rho, xs_xi - np.asarray(xi_nom, float)[None]], axis=-1)


def sample_covariance(e):
    """[N+1, 12, 12] over the first axis of e [S, N+1, 12], about the sample mean."""
    e = e - e.mean(axis=0, keepdims=True)
    return np.einsum("sia,sib->iab", e, e) / (e.shape[0] - 1)


def standard_errors(Sig, S):
    """se_ab = sqrt((S_aa S_bb + S_ab^2) / (S - 1)) of a Gaussian sample covariance of S samples, for Sig [..., 12, 12]."""
    d = np.einsum("...aa->...a", Sig)
    return np.sqrt((d[..., :, None] * d[..., None, :] + Sig ** 2) / (S - 1))


def gaussian_samples(rng, S0, W, V, mask, S, N):
    """(dx0 [S, 12], w [S, N, 6], n [S, N+1, 12]) for one trajectory: N(0, Sigma0), N(0, W), N(0, V) on the measured coordinates."""
    dx0 = rng.multivariate_normal(np.zeros(12), S0, size=S)
    w = rng.multivariate_normal(np.zeros(6), W, size=(S, N))
    sd = np.zeros(12)
    sd[measured(mask)] = np.sqrt(np.asarray(V, float)[measured(mask)])
    return dx0, w, rng.normal(size=(S, N + 1, 12)) * sd


def open_loop_policy(prob, q0, xi0, us, seed=3):
    """A policy the CPU can state without a solve (the construction of tests/test_covariance_cpu.py's _se3_policy): an open-loop
    rollout of the perturbed controls as the nominal (no defects), and the gains of the oracle's sweep about it.
    q0 [4, 4], xi0 [6], us [N, m].  Returns (op, q [N+1, 4, 4], xi [N+1, 6], u [N, m], K [N, m, 12])."""
    op = op_of(prob)
    N, m = us.shape
    rng = np.random.default_rng(seed)
    u = us + rng.normal(size=(N, m)) * 0.1
    q = np.zeros((N + 1, 4, 4)); xi = np.zeros((N + 1, 6))
    q[0], xi[0] = np.asarray(q0, float).reshape(4, 4), xi0
    for i in range(N):
        q[i + 1], xi[i + 1] = ob.f(op, q[i], xi[i], u[i])
    K = ob.lin_backward(op, q, xi, u, ms=False)["K"]
    return op, q, xi, u, K


def held_policy_cpu(prob, q0, xi0, us, mode):
    """The CPU twin of tests/support.py's held_policy for one trajectory: the oracle's solve with KW's four iterations and zero
    tolerances, then its sweep about the result.  Returns (op, q [N+1, 4, 4], xi [N+1, 6], u [N, m], K [N, m, 12])."""
    op = op_of(prob)
    o = ob.fit(op, np.asarray(q0, float).reshape(16), xi0, us, mode=mode, max_iter=KW["n_iterations"], tol_grad=0.0, tol_defect=0.0)
    q, xi, u = np.asarray(o["xs_q"]).reshape(-1, 4, 4), o["xs_xi"], o["us"]
    return op, q, xi, u, ob.lin_backward(op, q, xi, u, ms=(mode == "ms"))["K"]


# the masks of the GPU parity tests: pose only, and a mixed pattern; the SO3 family's carry no translation bits
MASKS = (0x03F, 0x5A5)
MASKS_SO3 = (0x007, 0x1C5)
MASKS_EDGE = (0x000, 0x001, 0x800, 0xFC0, 0xFFF)


def masks_of(prob):
    return MASKS_SO3 if prob.kind in ("so3", "pendulum3d") else MASKS


def estimated_inputs(prob, B, seed=7, sigma=0.005, noise=0.1):
    """(Sigma0, W, V) as the solver takes them and as the restatement reads them: (S0, W, V, S0r, Wr, Vr).  Sigma0 and W are
    tests/support.py's moment_inputs (so3 and the pendulum in compact form) at other scales; V = diag(Sigma0) * U[0.25, 4],
    seeded: a sensor between half and twice the start knowledge's standard deviation.  The scales -- start knowledge 0.005, twist
    disturbance 0.1 per step -- let the disturbance set max |Sigma|: with the start knowledge dominant (0.05 / 0.01) the drone's
    gains, 3e3, put var_u = diag K S^ K^T four decades above max |Sigma| and its rounding, eps |var_u|, at 4e-11 of max |Sigma|,
    over the 1e-11 that tests/test_estimated_cpu.py holds every output of these inputs to against long double."""
    rng = np.random.default_rng(seed + 11)
    if prob.kind in ("so3", "pendulum3d"):
        S0, W = psd(B, 6, sigma, seed), psd(B, 3, noise, seed + 1)
        V = np.einsum("bii->bi", S0) * rng.uniform(0.25, 4.0, (B, 6))
        Vr = np.zeros((B, 12))
        Vr[:, SO3_COORDS] = V
        return S0, W, V, embed(S0, SO3_COORDS, 12), embed(W, [0, 1, 2], 6), Vr
    S0, W = psd(B, 12, sigma, seed), psd(B, 6, noise, seed + 1)
    V = np.einsum("bii->bi", S0) * rng.uniform(0.25, 4.0, (B, 12))
    return S0, W, V, S0, W, V


ESTIMATED_FIELDS = ("J", "xs_q", "xs_xi", "us", "est_q", "est_xi")


def restate_estimated_batch(ops, nom, K, L, mask, dx0, w, n):
    """restate_rollout_estimated for every trajectory of a batch: a list of dicts over ESTIMATED_FIELDS.  ops: one OracleProblem
    per trajectory; nom: xs_q / xs_xi / us [B, ...] (numpy); K [B, N, m, 12]; L [B, N+1, 12, 12]; dx0, w, n [B, S, ...]."""
    with np.errstate(all="ignore"):
        return [dict(zip(ESTIMATED_FIELDS, restate_rollout_estimated(op, nom.xs_q[b], nom.xs_xi[b], nom.us[b], K[b], L[b], mask,
                                                                     dx0[b], w[b], n[b], dx0.shape[1])))
                for b, op in enumerate(ops)]


def estimated_guard(op, prob, nom, K, L, mask, dx0, w, n, least=4):
    """The coverage guard and the caps of the estimated loop at large rotations, on the restatement alone: every site of
    k_policy_rollout_est holds at least `least` samples in every tier of estimated_need (least = 0: not asked), counted over the
    samples the restatement determines (tests/support.py::determined, gains K and L moved in their last place); three quarters
    of the samples stay finite, and three quarters are determined.
    Returns (the restatement, keep [B, S], the spread per field [B, S])."""
    B, S = dx0.shape[:2]
    R = restate_estimated_batch([op] * B, nom, K, L, mask, dx0, w, n)
    rng = np.random.default_rng(5)
    sp = sample_spread(R, restate_estimated_batch([op] * B, nom, nudged(K, rng), nudged(L, rng), mask, dx0, w, n))
    keep = determined(sp)
    if least:
        tags = []
        for b in range(B):
            r = {f: v[keep[b]] for f, v in R[b].items()}
            tags += estimated_site_tags(op, prob, nom.xs_q[b], nom.xs_xi[b], L[b], mask, n[b][keep[b]],
                                        *(r[f] for f in ESTIMATED_FIELDS[1:]))
        assert_coverage(tags, need=estimated_need(prob.N, mask), least=least)
    fin = sum(int(np.isfinite(r["J"]).sum()) for r in R)
    assert 4 * fin >= 3 * B * S, (fin, B * S)
    assert 4 * int(keep.sum()) >= 3 * B * S, (int(keep.sum()), B * S)
    return R, keep, sp
