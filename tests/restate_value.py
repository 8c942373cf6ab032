"""Host restatement of tolg_policy_value from oracle primitives only (ob.fx_fu, ob.cost): what tests/test_value_cpu.py checks
on its own and tests/test_gpu_value.py checks the kernel against.  A plain module (pytest does not collect it)."""
import numpy as np

from oracle import bridge as ob


def _sym(a, n):
    return np.zeros((n, n)) if a is None else 0.5 * (np.asarray(a, float) + np.asarray(a, float).T)


def restate_stage_weights(op, q, xi, u, K):
    """M_i = l_xx + K_i^T l_uu K_i (i < N), M_N = l_xx^N at the nominal, symmetrised: [N+1, 12, 12]."""
    N = u.shape[0]
    M = np.zeros((N + 1, 12, 12))
    for i in range(N):
        _, _, lxx, _, luu = ob.cost(op, q[i], xi[i], u[i], i)
        M[i] = _sym(lxx + K[i].T @ luu @ K[i], 12)
    M[N] = _sym(ob.cost(op, q[N], xi[N], None, N, terminal=True)[2], 12)
    return M


def restate_value(op, q, xi, u, K, Sigma0=None, W=None, variant=None):
    """Cost-to-go of the policy (x*, u*, K) about its nominal: P_N = l_xx^N, p_N = l_x^N and, for i = N-1 .. 0,
      P_i = l_xx + K_i^T l_uu K_i + Acl_i^T P_{i+1} Acl_i,   p_i = l_x + K_i^T l_u + Acl_i^T p_{i+1},   Acl_i = f_x + f_u K_i,
      price_i = tr(P_{i+1}[6:12, 6:12] W) / 2,   excess = tr(P_0 Sigma0) / 2 + sum_i price_i.
    q [N+1, 4, 4], xi [N+1, 6], u [N, m], K [N, m, 12], Sigma0 [12, 12], W [6, 6] (None: zero).
    variant: a deliberately WRONG recursion for negative controls -- "no_Klu" drops K_i^T l_u from p, "untransposed" applies
    Acl_i where Acl_i^T belongs.
    Returns P [N+1, 12, 12], p [N+1, 12], diag_P [N+1, 12], price [N], excess."""
    assert variant in (None, "no_Klu", "untransposed")
    N = u.shape[0]
    S0, Wn = _sym(Sigma0, 12), _sym(W, 6)
    P = np.zeros((N + 1, 12, 12)); p = np.zeros((N + 1, 12)); price = np.zeros(N)
    _, lx, lxx, _, _ = ob.cost(op, q[N], xi[N], None, N, terminal=True)
    P[N], p[N] = _sym(lxx, 12), lx
    for i in range(N - 1, -1, -1):
        Fx, Fu = ob.fx_fu(op, q[i], xi[i], u[i])
        Acl = Fx + Fu @ K[i]
        At = Acl if variant == "untransposed" else Acl.T
        _, lx, lxx, lu, luu = ob.cost(op, q[i], xi[i], u[i], i)
        P[i] = _sym(lxx + K[i].T @ luu @ K[i] + At @ P[i + 1] @ At.T, 12)
        p[i] = lx + (0.0 if variant == "no_Klu" else K[i].T @ lu) + At @ p[i + 1]
        price[i] = 0.5 * np.trace(P[i + 1][6:, 6:] @ Wn)
    excess = 0.5 * np.trace(P[0] @ S0) + price.sum()
    return P, p, np.einsum("icc->ic", P).copy(), price, excess
