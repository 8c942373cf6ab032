"""Large-rotation parity of the production kernels with the oracle, across every tier of csrc/tolg_lie.h.

The case grid (tests/support.py: rotation_grid, large_rotation_problem, knot_states, large_rotation_trajectories) puts
deviations and step rotations on both sides of every threshold the kernels branch on, absolute orientations through all four
branches of R_to_q, and product quaternions with w < 0; every test asserts on the host, before it launches, that its states
reach the buckets it is about (assert_coverage), with R_to_q restated in numpy (r_to_q).

  a. tolg_eval_knot (lin_knot under its own gate, k_probe_pack, k_probe_export) against the oracle's per-knot functions, in
     a uniform layout (64 consecutive states of one bucket: a wave runs one tier) and a mixed one (every wave holds every
     bucket), and bitwise against the same state evaluated alone;
  b. tolg_linearize_backward (k_linearize on stored trajectories, the closed-form defect Log) against ob.lin_backward;
  c. tolg_rollout (k_rollout in its four forms and the merit step) against tests/restate.py::restate_rollout;
  d. tolg_policy_rollout with start perturbations and twist noise from the grid against restate_policy, in both sample orders.

Bounds.  The project's own: check_linearize_backward's (Fx 1e-12, d 1e-11, lx / lxx 1e-11, J 1e-12, K / k 1e-8), the pendulum
knot test's (f_q 1e-14 absolute, f_xi / Fx / Fu 1e-13) and check_restatement's (states 1e-10, inputs 1e-8, J 1e-9).  f_xi's
bound is relative to max(1, |f_xi|) as d's is: with |omega| dt up to 4 rad a twist entry reaches 1e3, where 1e-13 absolute is
less than one unit in the last place.  l_u and l_uu (2 R u, 2 R: m products each) take 1e-13, err takes d's bound.
A field keeps its bound where eight times the reference's own floor is below it; where it is not, the bound is eight times
the floor, in that bucket only.  Floors, all measured on the CPU on the states of these tests:
  - (a), (b): the distance of ob.lin_backward from oracle.bridge_ld.lin_backward (long double).  Outside two buckets the worst
    per-state figures are Fx 1.9e-15, l_x 4.0e-13, l_xx 2.6e-13 (whole trajectories of (b): Fx 2.3e-15, d 4.1e-13, l_x 1.1e-13,
    l_xx 4.8e-14, J 6.7e-16, K 4.8e-13, k 3.0e-13): every project bound stays.  The two buckets are small angles, where the
    fp64 ORACLE is the noisy side -- its closed-form coefficients such as (t^2 + 2 cos t - 2) / (2 t^4) cancel, the kernels'
    series do not (on the device the worst figures there EQUAL these floors: it agrees with the long-double oracle):
      "log_cancel", a deviation below 1e-2 rad: l_x 1.7e-10, l_xx 8.3e-11 per state, 1.2e-12 / 2.2e-12 per trajectory of (b);
      "exp_cancel", a step rotation between 1e-5 and 1e-2 rad: Fx 9.4e-12 per state, 7.3e-13 per trajectory of (b); f_q's
      translation 4.9e-13 from a long-double restatement of x.t + R V(omega dt) v dt (4.5e-16 outside the bucket).
    FLOOR below holds these figures; the bounds used are 8 x FLOOR in those buckets and the project's everywhere else.
  - the band within 2e-3 of pi is outside the element parity of (a): err's rotation part may come out with either sign
    (l_x floor there 5.6e-11); it is compared through Exp, and f, Fx, Fu, which do not depend on the deviation, as elsewhere.
  - (c), (d): the spread of the restatement under a relative perturbation of 1e-15 of its gains and start state.  (d): 1.1e-14 on
    poses, 3.6e-12 on twists, 5.1e-11 on inputs, 4.1e-15 on J at worst: check_restatement's bounds stay.  (c): see ROLLOUT_FLOOR
    below for the figures and for which rollouts are compared.
The worst figures of a GPU run are printed by every test and kept in profiles/large_rotation_parity.txt."""
import functools

import numpy as np
import pytest
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
from tests.checks import K1_FIELDS, check_linearize_backward, check_restatement
from tests.restate import restate_policy, restate_rollout
from tests.support import (EXP_TIERS, KNOT_BUCKETS, LOG_TIERS, MODELS, Nominal, assert_coverage, exp_tier, host, knot_states,
                           large_rotation_problem, large_rotation_trajectories, log_tier, model_case, op_of, policy_handle,
                           policy_perturbations, problem_of_kind, product_quaternion, rel, same, trajectory_buckets)

pytestmark = pytest.mark.gpu

# the reference's own floors (module docstring): fp64 oracle against long-double oracle, per state (a) and per trajectory (b)
FLOOR = {"state": {"lx": 1.7e-10, "lxx": 8.3e-11, "Fx": 9.4e-12, "f_q": 4.9e-13},
         "traj": {"lx": 1.2e-12, "lxx11": 2.2e-12, "Fx": 7.3e-13}}
N_A, KNOT_A = 22, 5      # (a): horizon and interior knot; both knot 5 and knot 22 track an orientation of 89 degrees about a
#                          negative axis, so that a small deviation carries a state across R_to_q's sign change
SEED = 600                # of the trajectories of (b), (c): chosen on the CPU so that the restatement keeps 3 of 4 rollouts finite
CALL = 256               # states per eval_knot call


def _worst(w, name, e):
    w[name] = max(w.get(name, 0.0), float(e))
    return e


def _show(what, w):
    print(what, {k: "%.1e" % v for k, v in sorted(w.items())})


# ---- a. tolg_eval_knot ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _knot_case(model, term):
    """The states of one (model, knot) with the oracle's values for them, computed once and left unchanged."""
    prob = large_rotation_problem(model_case(model, 1, N=N_A)[0])
    i = prob.N if term else KNOT_A
    ks = knot_states(prob, i)
    op = op_of(prob)
    ref = []
    for q, xi, u in zip(ks["x_q"], ks["x_xi"], ks["u"]):
        r = dict(zip(("l", "lx", "lxx", "lu", "luu"), ob.cost(op, q, xi, None if term else u, i, terminal=term)))
        r["err"] = np.r_[ob.lminus(q, prob.q_ref[i])[0], xi - prob.xi_ref[i]]
        if not term:
            r["f_q"], r["f_xi"] = ob.f(op, q, xi, u)
            r["Fx"], r["Fu"] = ob.fx_fu(op, q, xi, u)
        ref.append(r)
    return prob, i, ks, ref


def _eval(solver, i, ks, order):
    """eval_knot on the states in `order`, CALL at a time: {field: [n, ...]} on the host."""
    out = {}
    for a in range(0, len(order), CALL):
        sl = order[a:a + CALL]
        r = solver.eval_knot(i, ks["x_q"][sl], ks["x_xi"][sl], ks["u"][sl])
        torch.cuda.synchronize()
        for k, v in r.items():
            out.setdefault(k, []).append(host(v))
    return {k: np.concatenate(v) for k, v in out.items()}


def _state_bound(field, tags):
    if field in ("lx", "lxx") and "log_cancel" in tags:
        return 8 * FLOOR["state"][field]
    if field == "Fx" and "exp_cancel" in tags:
        return 8 * FLOOR["state"]["Fx"]
    if field == "f_q":
        return 8 * FLOOR["state"]["f_q"] if "exp_cancel" in tags else 1e-14
    return {"Fx": 1e-13, "Fu": 1e-13, "l": 1e-12, "lx": 1e-11, "lxx": 1e-11, "lu": 1e-13, "luu": 1e-13}[field]


@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("term", [False, True], ids=["interior", "terminal"])
@pytest.mark.parametrize("model", MODELS)
def test_eval_knot_matches_oracle_in_every_tier(model, term, layout):
    prob, i, ks, ref = _knot_case(model, term)
    assert_coverage(ks["tags"])
    n = len(ref)
    order = np.arange(n) if layout == "uniform" else ks["mixed"]
    if layout == "uniform":  # a wave is one bucket
        assert all(all(ks["waves"][j // 64] in ks["tags"][k] for k in range(j, j + 64)) for j in range(0, n, 64))
    else:                    # every block of 256 holds every bucket
        for a in range(0, n, CALL):
            assert_coverage([ks["tags"][k] for k in order[a:a + CALL]], least=1)
    got = _eval(BatchedTrackingILQR(prob, CALL), i, ks, order)
    w = {}
    for j, k in enumerate(order):
        r, t = ref[k], ks["tags"][k]
        g = {f: v[j] for f, v in got.items()}
        if not term:
            ec = ":exp_cancel" if "exp_cancel" in t else ""
            assert _worst(w, "f_q" + ec, np.abs(g["f_q"] - r["f_q"]).max()) < _state_bound("f_q", t), (k, t)
            assert _worst(w, "f_xi", np.abs(g["f_xi"] - r["f_xi"]).max() / max(1.0, np.abs(r["f_xi"]).max())) < 1e-13, (k, t)
            for f in ("Fx", "Fu"):
                assert _worst(w, f + (ec if f == "Fx" else ""), rel(g[f], r[f])) < _state_bound(f, t), (f, k, t)
        if "near_pi" in t:
            # Log's rotation part may come out with either sign this close to pi: compare the rotation it stands for
            assert np.linalg.norm(g["err"][:3]) <= np.pi + 1e-12
            assert _worst(w, "Exp(err):near_pi", np.abs(ob.se3_exp(g["err"][:6]) - ob.se3_exp(r["err"][:6])).max()) < 1e-9, (k, t)
            assert np.array_equal(g["err"][6:], r["err"][6:]) or rel(g["err"][6:], r["err"][6:]) < 1e-15
            continue
        assert _worst(w, "err", np.abs(g["err"] - r["err"]).max() / max(1.0, np.abs(r["err"]).max())) < 1e-11, (k, t)
        assert _worst(w, "l", abs(g["l"] / r["l"] - 1)) < 1e-12, (k, t)
        for f in ("lx", "lxx") + (() if term else ("lu", "luu")):
            lc = ":log_cancel" if f in ("lx", "lxx") and "log_cancel" in t else ""
            assert _worst(w, f + lc, rel(g[f], r[f])) < _state_bound(f, t), (f, k, t)
    _show("eval_knot %s %s %s" % (model, "terminal" if term else "interior", layout), w)


@pytest.mark.parametrize("term", [False, True], ids=["interior", "terminal"])
@pytest.mark.parametrize("model", MODELS)
def test_eval_knot_lane_gets_the_bits_it_gets_alone(model, term):
    """Every value is decided per lane (csrc/tolg_lie.h): a state evaluated with n = 1 -- the padded lanes replicate it, the
    wave is uniform -- gives the bits it gets at its place in the mixed call, in every output field, for a state of every
    bucket."""
    prob, i, ks, _ = _knot_case(model, term)
    assert_coverage(ks["tags"])
    order = ks["mixed"]
    s = BatchedTrackingILQR(prob, CALL)
    got = _eval(s, i, ks, order)
    for bucket in KNOT_BUCKETS + ("near_pi",):
        j = next(j for j, k in enumerate(order) if bucket in ks["tags"][k])
        one = _eval(s, i, ks, order[j:j + 1])
        assert set(one) == set(got)
        for f in got:
            assert np.array_equal(one[f][0].view(np.int64), got[f][j].view(np.int64)), (bucket, f, j)


# ---- b. tolg_linearize_backward -------------------------------------------------------------------------------------------
def _traj_case(kind, N, B, twists):
    prob = large_rotation_problem(problem_of_kind(kind, 1, N)[0])
    xs_q, xs_xi, us = large_rotation_trajectories(prob, B, seed=SEED + N + B, twists=twists)
    tags = trajectory_buckets(prob, xs_q, xs_xi)
    return prob, xs_q, xs_xi, us, tags


def _traj_guard(prob, B, tags, twists):
    """The coverage guard of (b) and (c); at N = 3 a batch has 4 B knots, and the guard asks for what they can hold."""
    need = LOG_TIERS + ("conv0", "conv1", "conv2", "conv3", "defect_large", "defect_wneg")
    if twists != "moderate":
        need += EXP_TIERS
    if prob.N >= 24:
        assert_coverage(tags, need=need, least=1 if twists == "sparse" and B < 17 else 4 if B >= 17 or twists == "moderate" else 2)
    else:
        assert_coverage(tags, need=("log_long", "log_closed", "defect_large", "defect_wneg", "conv0"), least=1)
    assert not any("defect_near_pi" in t for t in tags)   # d is compared element by element


def _traj_bounds(prob, B, tags):
    """Per trajectory: 8 x FLOOR for the fields a small-angle knot makes the oracle noisy in, the project's otherwise."""
    per = [set().union(*tags[b * (prob.N + 1):(b + 1) * (prob.N + 1)]) for b in range(B)]
    lc, ec = np.array(["log_cancel" in t for t in per]), np.array(["exp_cancel" in t for t in per])
    return {"lx": np.where(lc, max(1e-11, 8 * FLOOR["traj"]["lx"]), 1e-11),
            "lxx11": np.where(lc, max(1e-11, 8 * FLOOR["traj"]["lxx11"]), 1e-11),
            "Fx": np.where(ec, max(1e-12, 8 * FLOOR["traj"]["Fx"]), 1e-12)}


@pytest.mark.parametrize("twists", ["moderate", "tiers"])
@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("N", [24, 3])
@pytest.mark.parametrize("kind", ["se3", "drone", "so3"])
def test_linearize_backward_matches_oracle_in_every_tier(kind, N, B, twists):
    """moderate twists: the sweep stays clean, all of check_linearize_backward applies (K, k, grad, mu_delta included).  Step
    rotations across the Exp tiers: the sweep regularises up to max_reg on both sides, what K1 produces is compared."""
    prob, xs_q, xs_xi, us, tags = _traj_case(kind, N, B, twists)
    _traj_guard(prob, B, tags, twists)
    s = BatchedTrackingILQR(prob, B)
    for ms in (True, False):
        w = check_linearize_backward(prob, xs_q, xs_xi, us, ms, solver=s, fields=None if twists == "moderate" else K1_FIELDS,
                                     bounds=_traj_bounds(prob, B, tags))
        _show("linearize_backward %s N=%d B=%d %s ms=%d" % (kind, N, B, twists, ms), w)


# ---- c. tolg_rollout ------------------------------------------------------------------------------------------------------
# The restatement's own floor: its spread (largest absolute difference) when its gains and start twist move by 1e-15 relative.
# Measured on the CPU over the 1572 finite rollouts of these cases, with the oracle's gains: the median spread is 7e-16 on poses,
# 1.4e-15 on twists, 2.3e-15 on inputs; 99 in 100 stay below 1.8e-13 / 2.0e-14 / 2.3e-14; a few rollouts amplify it by 1e10 and more
# (closed loops about defects of radians; a deviation that passes pi, where rounding decides Log's sign, lands elsewhere).
# A rollout takes a rounding error of that size at each of its N steps, not at the start alone, so its floor is N times its spread.
# Where eight times that floor is below check_restatement's bounds (1e-10 states, 1e-8 inputs) the rollout is compared, to those
# bounds; where it is not, the restatement does not determine the rollout to the bounds and it counts as not kept, like one
# that is not finite: no bound is ever wider than the project's.  Of every (mode, form, alpha) at least 3 in 4 rollouts must be
# finite and at least 1 in 2 compared (the accept-always nonlinear step on se3, whose feed-forward of 1e4 closes defects of
# radians in one step, is the sensitive one: 10 of 17 there, all or all but a few elsewhere).  The spread is computed in the
# test, from the restatement alone, before the device's values are looked at.
ROLLOUT_FLOOR = 1e-15
ALPHAS = (1.0, 0.5, 1.1 ** -16)
GATE_CLASSES = ("small", "long", "closed")


def _gate_class(tier):
    return 0 if tier <= 1 and tier != 0 else 1 if tier == 2 else 2


def _rollout_gates(prob, q, xi, nq, nxi):
    """(Log class, Exp class) of roll_step's shared gate at every knot of one rollout: the deviation x_i^-1 x^_i and the step
    rotation of x^_i.  Classes: small, long, closed (tiny and beyond-pi arguments are outside the series' domain too)."""
    out = set()
    for i in range(prob.N):
        y = product_quaternion(nq[i], q[i], left=False)[1]
        th2 = prob.dt ** 2 * float(nxi[i, :3] @ nxi[i, :3])
        lt, et = log_tier(y), exp_tier(th2)
        out.add((0 if lt <= 1 else lt - 1, 2 if et == 0 else _gate_class(et)))   # a tiny Log is in domain, a tiny Exp is not
    return out


def _spread(fn, k, K, x0q, x0xi, rng):
    a = fn(k, K, x0q, x0xi)
    b = fn(k * (1 + ROLLOUT_FLOOR * rng.choice([-1, 1], k.shape)), K * (1 + ROLLOUT_FLOOR * rng.choice([-1, 1], K.shape)),
           x0q, x0xi * (1 + ROLLOUT_FLOOR * rng.choice([-1, 1], x0xi.shape)))
    return a, [np.abs(u - v).max() if np.isfinite(u).all() and np.isfinite(v).all() else np.inf for u, v in zip(a, b)]


@pytest.mark.parametrize("twists", ["moderate", "sparse"])
@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("kind", ["se3", "drone", "so3"])
def test_rollout_matches_restatement(kind, B, twists):
    """linearize_backward, then rollout(alpha, ms, form) in all twelve combinations, against restate_rollout with the device's
    gains.  alpha = 0.5 on multiple shooting is the merit step: the (alpha - 1) d conjugation under a gate of its own."""
    prob, xs_q, xs_xi, us, tags = _traj_case(kind, 24, B, twists)
    _traj_guard(prob, B, tags, twists)
    op = op_of(prob)
    s = BatchedTrackingILQR(prob, B)
    rng = np.random.default_rng(5)
    gates, w, total, finite = set(), {}, 0, 0
    for ms in (True, False):
        r = s.linearize_backward(xs_q, xs_xi, us, ms=ms)
        torch.cuda.synchronize()
        k, K = host(r["k"]), host(r["K"])
        for form in ("nonlinear", "linear"):
            for alpha in ALPHAS:
                g = [host(t) for t in s.rollout(B, alpha, ms, form)]
                ok = fin = 0
                for b in range(B):
                    with np.errstate(all="ignore"):
                        (nq, nxi, nu), sp = _spread(lambda k_, K_, q0, x0: restate_rollout(
                            op, np.r_[q0[None], xs_q[b, 1:]], np.r_[x0[None], xs_xi[b, 1:]], us[b], k_, K_, alpha, ms,
                            form == "linear"), k[b], K[b], xs_q[b, 0], xs_xi[b, 0], rng)
                    base = (1e-10, 1e-10, 1e-8)
                    if not (np.isfinite(nq).all() and np.isfinite(nxi).all() and np.isfinite(nu).all()):
                        continue   # diverged
                    fin += 1
                    if not all(8 * prob.N * v < c for v, c in zip(sp, base)):
                        continue   # not determined to the bounds by the restatement
                    ok += 1
                    gates |= _rollout_gates(prob, xs_q[b], xs_xi[b], nq, nxi)
                    what = (kind, B, twists, ms, form, alpha, b)
                    for name, got, ref, spr, c in (("xs_q", g[0][b], nq, sp[0], base[0]), ("xs_xi", g[1][b], nxi, sp[1], base[1]),
                                                   ("us", g[2][b], nu, sp[2], base[2])):
                        assert _worst(w, name, np.abs(got - ref).max()) < c, (name, what, spr)
                total += B; finite += ok
                assert 4 * fin >= 3 * B and 2 * ok >= B, (kind, B, twists, ms, form, alpha, fin, ok)
    # the shared gate log_small(yl) && exp_small(th2e) has seen every (Log class, Exp class) the set can hold
    want = {(a, b) for a in range(3) for b in range(3)} if twists == "sparse" else {(a, 0) for a in range(3)}
    assert want <= gates, sorted(want - gates)
    _show("rollout %s B=%d %s (%d of %d kept)" % (kind, B, twists, finite, total), w)


# ---- d. tolg_policy_rollout -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("kind", ["se3", "drone", "so3"])
def test_policy_rollout_with_large_perturbations(kind, N, layout):
    """roll_step<.., ALPHA1> and knot_cost<FAST> with 16 samples of one trajectory per wave; the short horizon keeps a 3 rad
    perturbation from diverging.  Both sample orders of k_policy_rollout give the same bits."""
    B, S = 5, 32
    prob = large_rotation_problem(problem_of_kind(kind, 1, N)[0])
    xs_q, xs_xi, us = large_rotation_trajectories(prob, B, seed=7 + N, twists="moderate")
    dx0, w = policy_perturbations(prob, B, S, layout, seed=11 + N)
    op = op_of(prob)
    # the coverage guard: the Log tier of every start deviation, the Exp tier of every step, from the restatement's samples
    tags = []
    for b in range(B):
        g = ob.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=True)
        _, xq, xx, _ = restate_policy(op, xs_q[b], xs_xi[b], us[b], g["K"], dx0[b], w[b], S)
        for smp in range(S):
            tags.append({LOG_TIERS[log_tier(product_quaternion(xq[smp, 0], xs_q[b, 0], left=False)[1])]} |
                        {EXP_TIERS[exp_tier(prob.dt ** 2 * float(xx[smp, i, :3] @ xx[smp, i, :3]))] for i in range(N + 1)
                         if np.isfinite(xx[smp, i]).all()})
        if layout == "uniform":   # a 16-sample group is one Log tier
            assert all(len({log_tier(np.sin(np.linalg.norm(d[:3]) / 2) ** 2) for d in dx0[b, a:a + 16]}) == 1 for a in (0, 16))
    assert_coverage(tags, need=LOG_TIERS + EXP_TIERS[1:])
    out = []
    for fast in (False, True):
        s = policy_handle(prob, B, fast)
        s.linearize_backward(xs_q, xs_xi, us, ms=True)
        check_restatement(s, Nominal(xs_q, xs_xi, us), [op] * B, dx0, w, min_finite=(3, 4))
        out.append(s.policy_rollout(dx0, w, trajectories=True))
    for f in ("J", "status", "xs_q", "xs_xi", "us"):
        assert same(getattr(out[0], f), getattr(out[1], f)), f
