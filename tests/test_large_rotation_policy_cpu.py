"""CPU twin of tests/test_gpu_large_rotation_policy.py: on the restatements alone, with the oracle's gains, every coverage
guard, cap and condition of its cases A to C, the spread of the restatements that its bounds rest on, and the long-double floor
of the covariance and value recursions.  A case whose inputs stop exercising what it is about fails here, on any machine."""
import numpy as np
import pytest

from oracle import bridge as ob
from oracle import bridge_ld as ld
from tests.checks import limited_guard
from tests.estimated import estimated_guard
from tests.restate import restate_covariance, restate_value
from tests.support import (POLICY_B, POLICY_S, VALUE_B, box_widen, large_estimated_case, large_policy_case, large_value_case,
                           moment_inputs, op_of, value_guard, worst_spread)

KINDS = ["se3", "drone", "so3"]
LD = np.longdouble


def oracle_gains(op, nom):
    return np.array([ob.lin_backward(op, nom.xs_q[b], nom.xs_xi[b], nom.us[b], ms=True)["K"] for b in range(nom.us.shape[0])])


def _show(what, keep, sp):
    print("%s: %d of %d samples determined, spread over them %s" % (what, int(keep.sum()), keep.size,
                                                                    {k: "%.1e" % v for k, v in worst_spread(sp, keep).items()}))


# ---- A. the estimated loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose_only", [False, True], ids=["all", "pose"])
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_estimated_loop_inputs_reach_every_site_and_tier(kind, N, layout, pose_only):
    prob, nom, dx0, w, n, mask, L = large_estimated_case(kind, N, layout, pose_only)
    op = op_of(prob)
    R, keep, sp = estimated_guard(op, prob, nom, oracle_gains(op, nom), L, mask, dx0, w, n)
    assert sum(int(np.isfinite(r["J"]).sum()) for r in R) == POLICY_B * POLICY_S   # with the oracle's gains every sample is finite
    _show("estimated %s N=%d %s %#05x" % (kind, N, layout, mask), keep, sp)


def test_estimated_loop_ragged_case_keeps_its_samples():
    prob, nom, dx0, w, n, mask, L = large_estimated_case("se3", 4, "mixed", False, S=7)
    op = op_of(prob)
    R, keep, sp = estimated_guard(op, prob, nom, oracle_gains(op, nom), L, mask, dx0, w, n, least=0)
    _show("estimated ragged", keep, sp)


# ---- B. the limited loop ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_limited_loop_inputs_meet_the_conditions_in_every_tier(kind, N, layout):
    prob, nom, dx0, w = large_policy_case(kind, N, layout)
    op = op_of(prob)
    lb, ub, R, keep, sp = limited_guard(op, prob, nom, oracle_gains(op, nom), dx0, w, box_widen(kind, N))
    _show("limited %s N=%d %s" % (kind, N, layout), keep, sp)


# ---- C. covariance and value -----------------------------------------------------------------------------------------------
def covariance_ld(Fx, Fu, K, Sigma0, W):
    """restate_covariance's recursion in long double on given Jacobians: Fx [N, 12, 12] long double, Fu [N, 12, m]."""
    N = Fx.shape[0]
    Sig = np.zeros((N + 1, 12, 12), LD)
    Sig[0] = 0.5 * (Sigma0.astype(LD) + Sigma0.astype(LD).T)
    EW = np.zeros((12, 12), LD)
    EW[6:, 6:] = 0.5 * (W.astype(LD) + W.astype(LD).T)
    for i in range(N):
        Acl = Fx[i] + Fu[i].astype(LD) @ K[i].astype(LD)
        S = Acl @ Sig[i] @ Acl.T + EW
        Sig[i + 1] = 0.5 * (S + S.T)
    return Sig


def value_ld(Fx, Fu, Lx, Lxx, lu, luu, K):
    """restate_value's recursion for P and p in long double on given derivatives (Fx, Lx, Lxx long double)."""
    N = Fx.shape[0]
    P = np.zeros((N + 1, 12, 12), LD); p = np.zeros((N + 1, 12), LD)
    P[N], p[N] = 0.5 * (Lxx[N] + Lxx[N].T), Lx[N]
    for i in range(N - 1, -1, -1):
        Ki = K[i].astype(LD)
        Acl = Fx[i] + Fu[i].astype(LD) @ Ki
        M = Lxx[i] + Ki.T @ luu[i].astype(LD) @ Ki + Acl.T @ P[i + 1] @ Acl
        P[i] = 0.5 * (M + M.T)
        p[i] = Lx[i] + Ki.T @ lu[i].astype(LD) + Acl.T @ p[i + 1]
    return P, p


@pytest.mark.parametrize("ms", [True, False], ids=["ms", "ss"])
@pytest.mark.parametrize("twists", ["sparse", "tiers"])
@pytest.mark.parametrize("kind", KINDS)
def test_covariance_and_value_floor_on_large_rotation_nominals(kind, twists, ms):
    """The fp64 restatements against the same recursions carried in long double on oracle.bridge_ld.lin_backward's F_x, l_x and
    l_xx (F_u = B dt and l_u = 2 R u, l_uu = 2 R hold no series and come from the fp64 oracle; the gains are the fp64 oracle's on
    both sides).  Eight times the distance stays below the 1e-9 the device is held to, on every trajectory."""
    prob, xs_q, xs_xi, us, tags = large_value_case(kind, twists)
    value_guard(tags, twists)
    op = op_of(prob)
    _, _, S0r, Wr = moment_inputs(prob, VALUE_B)
    N = prob.N
    worst, kept = dict(Sigma=0.0, P=0.0, p=0.0), 0
    for b in range(VALUE_B):
        K = ob.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=ms)["K"]
        if not np.isfinite(K).all():
            continue
        kept += 1
        o = ld.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=ms)
        Fu = np.array([ob.fx_fu(op, xs_q[b, i], xs_xi[b, i], us[b, i])[1] for i in range(N)])
        c = [ob.cost(op, xs_q[b, i], xs_xi[b, i], us[b, i], i) for i in range(N)]
        Sig = restate_covariance(op, xs_q[b], xs_xi[b], us[b], K, S0r[b], Wr[b])[0]
        P, p = restate_value(op, xs_q[b], xs_xi[b], us[b], K, S0r[b], Wr[b])[:2]
        Pl, pl = value_ld(o["Fx"], Fu, o["Lx"], o["Lxx"], np.array([x[3] for x in c]), np.array([x[4] for x in c]), K)
        worst["Sigma"] = max(worst["Sigma"], float(np.abs(Sig - covariance_ld(o["Fx"], Fu, K, S0r[b], Wr[b])).max() / np.abs(Sig).max()))
        worst["P"] = max(worst["P"], float(np.abs(P - Pl).max() / np.abs(P).max()))
        worst["p"] = max(worst["p"], float(np.abs(p - pl).max() / np.abs(P).max()))
    print("floor %s %s ms=%d: %d of %d kept, %s" % (kind, twists, ms, kept, VALUE_B, {k: "%.1e" % v for k, v in worst.items()}))
    assert 4 * kept >= 3 * VALUE_B
    for k, v in worst.items():
        assert 8 * v < 1e-9, (k, v)
