"""The recipe table of tests/test_gpu_poison.py: every family of calls the library offers, each as a function
recipe(make_solver) -> dict[str, Tensor] that builds its handle and makes its calls, and returns every tensor the calls hand
back.  The tests run a recipe under tests/poison.py's three patterns: the handle's workspace, the buffers its setters pack into
and every output tensor are then born poisoned, and an output that depends on memory the library never wrote differs between
the patterns.

A plain module (pytest does not collect it): tests/test_gpu_poison.py, tests/test_poison_cpu.py and the TOLG_POISON_LDS child
process import it.  It imports one test module itself, tests/test_gpu_shapes.py, for the SWEEP table, its _model and its
_against_oracle, which are taken from there and not copied.  Importing it needs no GPU; running a recipe does.

All recipes use B = 5 trajectories on a handle of max_batch = 9: the call strides the workspace with Bp = 8 (one real lane in
the second group of four, three padded lanes) inside arrays carved for Bp = 12, so a tail of every array is never strided
over.  N = 5 everywhere, N = 25 as well for the solves (past the 24-knot state ring and the 4-deep rings), S = 3 samples.

Each recipe carries `reaches`, the C entry points its calls go through (tests/test_poison_cpu.py holds the table against
include/tolg.h), and optionally `oracle(make_solver, out)`: the oracle or restatement check the suite applies to that call,
with the bounds of the helper it comes from, run under the MINUS pattern.  A family without such a helper says so in its
docstring; bitwise agreement between the patterns is then its only assertion.

What an oracle hook compares depends on the helper.  The tensors the recipe returned (`out`, the MINUS run's) are themselves
held to the reference in the sweep, solve_*, held_refs, held_weights, held_box_*, al_fit_shared_box, al_mpc_step and mpc_measure
recipes.  The helpers that make their own call (check_linearize_backward, check_restatement, check_advance, check_loop,
compare_limited, compare_estimated and the actuated comparison) are not restated here: their hook repeats the call under MINUS
on another poisoned handle -- check_linearize_backward with the default mu and delta, check_loop on a handle of max_batch 5 --
so there the returned tensors are held to the reference only through the bitwise agreement of the three runs."""
import numpy as np
import torch

from oracle import bridge as ob
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, _capi, actuator_state, workloads
from tests import box as bx
from tests import kinds as kd
from tests import margins as mg
from tests import pose_kinds as pk
from tests.actuator import restate_policy_actuated
from tests.checks import (al_oracle, check_advance, check_linearize_backward, check_loop, check_restatement, compare_estimated,
                          compare_limited)
from tests.estimated import restate_rollout_estimated
from tests.limits import near_bound, restate_limited_batch
from tests.mpc_al import al_mpc_step_restated, g_box, g_spheres
from tests.mpc_estimated import restate_measure
from tests.schedule import distinct_schedule
from tests.support import RESULT_FIELDS, Nominal, host, op_of, pert, psd, random_traj, rel
from tests.support import ZERO as TOL0
from tests.test_gpu_shapes import SWEEP, _against_oracle, _model

B, MAXB, S, N_SHORT, N_LONG = 5, 9, 3, 5, 25
# every C entry point a recipe reaches through the constructor and the per-call bookkeeping of the Python layer
ALWAYS = ("tolg_create",)
SOLVE = ("tolg_solve_begin", "tolg_solve_iterate_until", "tolg_solve_iterate", "tolg_solve_end")

RECIPES = []


def recipe(name, reaches, oracle=None):
    def wrap(fn):
        fn.name, fn.reaches, fn.oracle = name, ALWAYS + tuple(reaches), oracle
        RECIPES.append(fn)
        return fn
    return wrap


def make_solver(prob):
    return BatchedTrackingILQR(prob, MAXB)


def f64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


def fields(r, prefix="", names=RESULT_FIELDS):
    """The tensors of a result object (or dict) under prefix + field name; a field that is None is left out."""
    get = (lambda k: r.get(k)) if isinstance(r, dict) else (lambda k: getattr(r, k, None))
    return {prefix + k: get(k) for k in names if isinstance(get(k), torch.Tensor)}


def tensors(obj, prefix=""):
    """Every tensor attribute of a result object, or entry of a dict"""
    items = obj.items() if isinstance(obj, dict) else vars(obj).items()
    return {prefix + k: v for k, v in items if isinstance(v, torch.Tensor)}


def mults(shape, seed, dev, lam=0.2, imu=2.0):
    """Seeded multipliers lambda >= 0 and I_mu >= 0 with some of each exactly zero: (numpy pair, device pair)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, lam, shape) * (rng.uniform(size=shape) > 0.2)
    b = rng.uniform(0.0, imu, shape) * (rng.uniform(size=shape) > 0.2)
    return (a, b), (f64(a, dev), f64(b, dev))


# ---- solves ---------------------------------------------------------------------------------------------------------------
def _sweep_recipe(row, name, kw, K, N):
    what = "%s %s N=%d" % (name, kw, N)

    def run(make):
        prob, q, xi, us = _model(name, B, N)
        return fields(make(prob).fit_batch(q, xi, us, n_iterations=K, **TOL0, **kw))

    def oracle(make, out):
        prob, q, xi, us = _model(name, B, N)
        o = ob.fit_batch(op_of(prob), q, xi, us, max_iter=K, mode=kw["mode"], line_search=kw.get("line_search", False),
                         rollout=kw.get("rollout", "nonlinear"))
        _against_oracle(out, o, 1e-8 if kw.get("line_search", False) or kw["mode"] == "ss" else 1e-9, what)

    run.__doc__ = "fit_batch, row %d of tests/test_gpu_shapes.py::SWEEP (%s), against the CPU oracle" % (row, what)
    recipe("sweep%02d_%s_N%d" % (row, name, N), SOLVE, oracle)(run)


for _N in (N_SHORT, N_LONG):
    for _row, (_name, _kw, _K) in enumerate(SWEEP):
        _sweep_recipe(_row, _name, _kw, _K, _N)


def _oracle_se3(K, **kw):
    """_against_oracle on the short se3 problem with the sweep's bound on J: 1e-8 for a solve that searches, else 1e-9"""
    tol = 1e-8 if kw.get("line_search", False) or kw["mode"] == "ss" else 1e-9

    def oracle(make, out, key=""):
        prob, q, xi, us = _model("se3", B, N_SHORT)
        o = ob.fit_batch(op_of(prob), q, xi, us, max_iter=K, **kw)
        _against_oracle({k[len(key):]: v for k, v in out.items() if k.startswith(key)}, o, tol, "se3 %s" % (kw,))
    return oracle


@recipe("solve_stepwise", ("tolg_solve_begin", "tolg_solve_iterate", "tolg_solve_peek", "tolg_solve_active_count",
                           "tolg_solve_iterate_until", "tolg_solve_end"),
        lambda make, out: _oracle_se3(4, mode="ms", line_search=True)(make, out, "end_"))
def solve_stepwise(make):
    """solve_begin / solve_iterate / solve_peek / active_count / solve_iterate_until / solve_end of the merit search (a solve
    that can stop, so that iterate_until counts on the device); the end result against the CPU oracle."""
    prob, q, xi, us = _model("se3", B, N_SHORT)
    s = make(prob)
    s.solve_begin(q, xi, us, mode="ms", n_iterations=4, line_search=True, **TOL0)
    s.solve_iterate(2)
    out = {k: v.clone() for k, v in fields(s.solve_peek(), "peek_").items()}
    out["active"] = torch.tensor([s.active_count()], dtype=torch.int32, device=s.device)
    s.solve_iterate_until(2, 1)
    out.update(fields(s.solve_end(), "end_"))
    return out


def _ref_states(prob):
    return (np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy(), np.broadcast_to(prob.xi_ref, (B,) + prob.xi_ref.shape).copy())


@recipe("solve_warm", ("tolg_solve_begin_warm", "tolg_solve_iterate_until", "tolg_solve_iterate", "tolg_solve_end"),
        lambda make, out: _oracle_se3(6, mode="ms")(make, out, "ref_"))
def solve_warm(make):
    """tolg_solve_begin_warm: shooting states near the reference on one handle (bitwise only: the oracle has no warm start), and
    on another the reference itself as the warm start, which is the cold solve's initial guess: against the CPU oracle."""
    prob, q, xi, us = _model("se3", B, N_SHORT)
    xq, xx, _ = random_traj(prob, B, seed=31, spread=0.1)
    out = fields(make(prob).fit_batch(q, xi, us, mode="ms", n_iterations=6, xs_init=(xq, xx), **TOL0), "near_")
    out.update(fields(make(prob).fit_batch(q, xi, us, mode="ms", n_iterations=6, xs_init=_ref_states(prob), **TOL0), "ref_"))
    return out


@recipe("solve_one_call", ("tolg_solve_batch",), _oracle_se3(4, mode="ss"))
def solve_one_call(make):
    """tolg_solve_batch (single shooting, slices of two iterations with the count read back), against the CPU oracle."""
    prob, q, xi, us = _model("se3", B, N_SHORT)
    return fields(make(prob).solve_batch_one_call(q, xi, us, mode="ss", n_iterations=4, check_every=2, **TOL0))


# ---- unit entry points as the very first call on the handle -------------------------------------------------------------
LIN_FIELDS = ("Fx", "d", "lx", "lxx11", "k", "K", "J", "dnorm", "grad", "mu_delta")


def _unit_traj(name):
    """test_linearize_backward_at_short_horizons' trajectories: random about the reference, the embedding's unused coordinates zero"""
    prob = _model(name, B, N_SHORT)[0]
    xs_q, xs_xi, us = random_traj(prob, B, seed=11 + N_SHORT)
    if name in ("so3", "pendulum"):
        xs_q[..., :3, 3] = 0.0
        xs_xi[..., 3:] = 0.0
        us[..., 3:] = 0.0
    return prob, xs_q, xs_xi, us


MU_DELTA_ARG = 6  # d_mu_delta among tolg_linearize_backward's arguments behind the handle (include/tolg.h)


def _lin_without_mu_delta(s, xs_q, xs_xi, us, ms):
    """BatchedTrackingILQR.linearize_backward with d_mu_delta = NULL: the binding always passes the array, so its one C call is
    made with that argument replaced (mu = 1, delta = 2 inside the library, nothing exported; the mu_delta tensor the binding
    returns is its own and left out)."""
    call = s._call

    def without(fn, *args, **kw):
        if fn != "tolg_linearize_backward":
            return call(fn, *args, **kw)
        return call(fn, *args[:MU_DELTA_ARG], None, *args[MU_DELTA_ARG + 1:], **kw)

    s._call = without
    try:
        r = s.linearize_backward(xs_q, xs_xi, us, ms=ms)
    finally:
        del s._call
    return {k: v for k, v in r.items() if k != "mu_delta"}


def _unit_recipe(name, ms, with_md):
    def run(make):
        prob, xs_q, xs_xi, us = _unit_traj(name)
        s = make(prob)
        r = s.linearize_backward(xs_q, xs_xi, us, ms=ms, mu=0.5, delta=3.0) if with_md else _lin_without_mu_delta(s, xs_q, xs_xi, us, ms)
        out = fields(r, "lin_", LIN_FIELDS)
        for alpha in (1.0, 0.5):
            for form in ("nonlinear", "linear"):
                a = s.rollout(B, alpha=alpha, ms=ms, rollout=form)
                out.update({"roll_%s_%g_%s" % (form, alpha, k): v for k, v in zip(("xs_q", "xs_xi", "us"), a)})
        if ms:
            for form in ("statement", "ring", "auto"):
                ecc, flag = s.expected_change(B, form)
                out.update({"ec_%s" % form: ecc, "ec_flag_%s" % form: flag})
        return out

    def oracle(make, out):
        prob, xs_q, xs_xi, us = _unit_traj(name)
        check_linearize_backward(prob, xs_q, xs_xi, us, ms, solver=make(prob))

    run.__doc__ = ("tolg_linearize_backward (%s, ms=%s, mu_delta %s) as the first call on its handle, then tolg_rollout at alpha "
                   "1 and 0.5, statement and linear, and tolg_expected_change in its forms, on that handle.  The oracle check is "
                   "check_linearize_backward's, as the first call on another handle; the rollouts and the expected change have "
                   "no oracle helper that takes a handle." % (name, ms, "given" if with_md else "NULL"))
    recipe("unit_%s_%s_%s" % (name, "ms" if ms else "ss", "md" if with_md else "nomd"),
           ("tolg_linearize_backward", "tolg_rollout") + (("tolg_expected_change",) if ms else ()), oracle)(run)


for _name in ("se3", "drone", "so3", "dense", "pendulum"):
    for _ms in (True, False):
        for _md in (True, False):
            _unit_recipe(_name, _ms, _md)


@recipe("eval_knot", ("tolg_eval_knot",))
def eval_knot(make):
    """tolg_eval_knot at an interior knot and at the terminal knot, each as the first call on its handle (se3 and the drone).  No
    oracle helper takes a handle for it: bitwise only."""
    out = {}
    for name in ("se3", "drone"):
        prob, xs_q, xs_xi, us = _unit_traj(name)
        for i in (2, N_SHORT):
            r = make(prob).eval_knot(i, xs_q[:, i], xs_xi[:, i], None if i == N_SHORT else us[:, i])
            out.update(tensors(r, "%s_%d_" % (name, i)))
    return out


def _held(make, name="se3", mode="ms", **per_traj):
    """A handle with a held policy: four accept-always iterations on the model's short problem.  Returns (prob, s, r, q, xi, us)."""
    prob, q, xi, us = _model(name, B, N_SHORT)
    s = make(prob)
    r = s.fit_batch(q, xi, us, mode=mode, n_iterations=4, **TOL0, **per_traj)
    return prob, s, r, q, xi, us


@recipe("solve_gains", SOLVE + ("tolg_solve_gains",))
def solve_gains(make):
    """tolg_solve_gains after a solve (se3 and the drone).  The gains enter check_restatement in the policy_rollout recipe; on
    their own there is no oracle helper: bitwise only."""
    out = {}
    for name in ("se3", "drone"):
        s = _held(make, name)[1]
        out.update(tensors(s.gains(), name + "_"))
    return out


# ---- held inputs ------------------------------------------------------------------------------------------------------------
FIT = dict(mode="ms", n_iterations=3, **TOL0)


def _se3():
    return workloads.se3_tracking(B, N=N_SHORT, R_scale=1e-3)


def _per_traj_oracle(ops, q, xi, us, what):
    def oracle(make, out):
        for b, op in enumerate(ops()):
            o = ob.fit_batch(op, q[b:b + 1], xi[b:b + 1], us[b:b + 1], max_iter=3, mode="ms")
            _against_oracle({k: v[b:b + 1] for k, v in out.items()}, o, 1e-9, "%s b=%d" % (what, b))
    return oracle


def _multiref():
    return workloads.se3_multiref(B, 3, N=N_SHORT)[:6]


def _weights(prob):
    f = 1.0 + 0.25 * np.arange(B)[:, None, None]
    return f * prob.Q[None], (2.0 - 0.1 * f) * prob.P[None], f * prob.R[None]


def _refs_oracle(make, out):
    prob, q, xi, us, q_ref, xi_ref = _multiref()
    _per_traj_oracle(lambda: [op_of(prob, q_ref[b], xi_ref[b]) for b in range(B)], q, xi, us, "refs")(make, out)


@recipe("held_refs", SOLVE + ("tolg_set_refs",), _refs_oracle)
def held_refs(make):
    """A reference per trajectory (tolg_set_refs), against the CPU oracle trajectory by trajectory."""
    prob, q, xi, us, q_ref, xi_ref = _multiref()
    return fields(make(prob).fit_batch(q, xi, us, q_ref=q_ref, xi_ref=xi_ref, **FIT))


def _weights_oracle(make, out):
    prob, q, xi, us = _se3()
    Q, P, R = _weights(prob)
    _per_traj_oracle(lambda: [op_of(prob, Q=Q[b], R=R[b], P=P[b]) for b in range(B)], q, xi, us, "weights")(make, out)


@recipe("held_weights", SOLVE + ("tolg_set_weights",), _weights_oracle)
def held_weights(make):
    """Cost weights per trajectory (tolg_set_weights), against the CPU oracle trajectory by trajectory."""
    prob, q, xi, us = _se3()
    Q, P, R = _weights(prob)
    return fields(make(prob).fit_batch(q, xi, us, Q=Q, P=P, R=R, **FIT))


@recipe("held_schedule", SOLVE + ("tolg_set_weights", "tolg_set_pose_schedule"))
def held_schedule(make):
    """A pose schedule (tolg_set_pose_schedule on the problem's own weights).  Its reference side is a host solve on a cost plugin
    (tests/schedule.py), not an oracle helper that takes these outputs: bitwise only."""
    prob, q, xi, us = _se3()
    return fields(make(prob).fit_batch(q, xi, us, pose_scale=distinct_schedule(B, N_SHORT), **FIT))


def _box(form, m=6):
    """Distinct bounds in the three forms a box is held in, and the same bounds as [B, N, m]"""
    lb, ub = bx.distinct_box(B, N_SHORT, m, seed=12)
    if form == "shared":
        lb, ub = np.ascontiguousarray(lb[0, 0]), np.ascontiguousarray(ub[0, 0])
        return lb, ub, np.broadcast_to(lb, (B, N_SHORT, m)).copy(), np.broadcast_to(ub, (B, N_SHORT, m)).copy()
    if form == "trajectory":
        lb, ub = np.ascontiguousarray(lb[:, 0]), np.ascontiguousarray(ub[:, 0])
        return lb, ub, np.repeat(lb[:, None], N_SHORT, 1), np.repeat(ub[:, None], N_SHORT, 1)
    return lb, ub, lb, ub


def _box_recipe(form):
    def run(make):
        prob, q, xi, us0 = _se3()
        xs_q, xs_xi, us = random_traj(prob, B, seed=11)
        lb, ub, lbk, ubk = _box(form)
        s = make(prob)
        _, (lam_d, imu_d) = mults((B, N_SHORT, 12), 13, s.device, lam=1.0, imu=20.0)
        s.set_al(lb, ub, lam_d, imu_d)
        out = fields(s.linearize_backward(xs_q, xs_xi, us, ms=True), "lin_", LIN_FIELDS)
        out.update(fields(s.fit_batch(q, xi, us0, **FIT), "fit_"))
        s.set_al(None)
        return out

    def oracle(make, out):
        """tests/test_gpu_input_box.py::test_linearize_backward_against_the_oracle's comparison, through the identity of
        tests/box.py, at its bounds (LIN_BOUNDS)"""
        prob, q, xi, us0 = _se3()
        xs_q, xs_xi, us = random_traj(prob, B, seed=11)
        lb, ub, lbk, ubk = _box(form)
        (lam, imu), _ = mults((B, N_SHORT, 12), 13, "cpu", lam=1.0, imu=20.0)
        g = g_box(us, lbk, ubk)
        assert (g > 0).any() and (g < 0).any()
        for b in range(B):
            op, const = bx.shifted_op(prob, lbk[b], ubk[b], lam[b], imu[b])
            o = ob.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=True)
            fig = dict(k=rel(host(out["lin_k"][b]), o["k"]), K=rel(host(out["lin_K"][b]), o["K"]),
                       lx=rel(host(out["lin_lx"][b]), o["Lx"]), J=abs(float(out["lin_J"][b]) / (o["J"] + const.sum()) - 1.0))
            for name, v in fig.items():
                assert v < bx.LIN_BOUNDS[name], (form, name, b, v)

    run.__doc__ = ("The input box held as %s (tolg_set_al%s): tolg_linearize_backward against the oracle through the identity of "
                   "tests/box.py, then a solve under it (bitwise)." % (form, "" if form == "shared" else "_box"))
    recipe("held_box_%s" % form, SOLVE + ("tolg_set_al" if form == "shared" else "tolg_set_al_box", "tolg_set_al", "tolg_linearize_backward"),
           oracle)(run)


for _form in ("shared", "trajectory", "knot"):
    _box_recipe(_form)


def _ref_poses(prob):
    return np.broadcast_to(prob.q_ref, (B,) + prob.q_ref.shape).copy()


def _spheres(prob, kinds, seed, moving=False):
    return kd.mixed_slots(_ref_poses(prob)[..., :3, 3], kinds, seed, moving=moving)


def _obstacle_recipe(name, kinds, moving, reaches):
    @recipe(name, SOLVE + reaches)
    def run(make):
        prob, q, xi, us = _se3()
        s = make(prob)
        obs = _spheres(prob, kinds, seed=21, moving=moving)
        _, (lam, imu) = mults((B, N_SHORT + 1, len(kinds)), 22, s.device)
        s.set_al_obstacles(obs, lam, imu, kinds=kinds if any(kinds) else None)
        out = fields(s.fit_batch(q, xi, us, **FIT))
        s.set_al_obstacles(None)
        return out
    run.__doc__ = ("A solve under %d %s position slots of kinds %s with fixed multipliers.  The suite's reference for it is a host "
                   "solve on the mirror's generic path, not an oracle helper on these outputs: bitwise only."
                   % (len(kinds), "moving" if moving else "static", kinds))


_obstacle_recipe("held_spheres_K1", (0,), False, ("tolg_set_al_obstacles",))
_obstacle_recipe("held_spheres_Kmax", (0,) * _capi.MAX_OBSTACLES, False, ("tolg_set_al_obstacles",))
_obstacle_recipe("held_spheres_moving", (0, 0), True, ("tolg_set_al_obstacles_moving",))
_obstacle_recipe("held_obstacle_kinds", kd.CORRIDOR, False, ("tolg_set_al_obstacles", "tolg_set_al_obstacle_kinds"))
_obstacle_recipe("held_obstacle_kinds_moving", kd.CORRIDOR, True, ("tolg_set_al_obstacles_moving", "tolg_set_al_obstacle_kinds"))


def _pose_recipe(name, per_knot):
    @recipe(name, SOLVE + ("tolg_set_al_pose_constraints",))
    def run(make):
        prob, q, xi, us = _se3()
        s = make(prob)
        slots = pk.mixed_slots(_ref_poses(prob), pk.MIXED, seed=23, per_knot_form=per_knot)
        _, (lam, imu) = mults((B, N_SHORT + 1, len(pk.MIXED)), 24, s.device)
        s.set_al_pose_constraints(slots, pk.MIXED, lam, imu)
        out = fields(s.fit_batch(q, xi, us, **FIT))
        s.set_al_pose_constraints(None)
        return out
    run.__doc__ = ("A solve under tilt and view cones (%s) with fixed multipliers.  As for the position slots the suite's "
                   "reference is a host solve: bitwise only." % ("per knot" if per_knot else "static"))


_pose_recipe("held_pose_static", False)
_pose_recipe("held_pose_per_knot", True)


def _paths(T=9):
    """World time for the *_windows setters on the short se3 problem: the problem's own reference path continued to T + 1 knots
    for every trajectory (the solves start near it), phases t0 in 0..2; the recipes gather step t = 1."""
    prob, q, xi, us = _se3()
    long = workloads.se3_tracking(1, N=T, R_scale=1e-3)[0]
    pq = np.broadcast_to(long.q_ref, (B,) + long.q_ref.shape).copy()
    px = np.broadcast_to(long.xi_ref, (B,) + long.xi_ref.shape).copy()
    return prob, q, xi, us, pq, px, np.array([0, 1, 2, 0, 1], dtype=np.int32)


@recipe("windows_refs", ("tolg_set_ref_windows", "tolg_solve_begin", "tolg_solve_iterate", "tolg_solve_end"))
def windows_refs(make):
    """tolg_set_ref_windows, then the solve the MPC loop begins behind it (a batch call of the Python layer would state its own
    references).  check_loop covers the call inside mpc(); alone it has no oracle helper: bitwise only."""
    prob, q, xi, us, pq, px, t0 = _paths()
    s = make(prob)
    b = s._stage(q, xi, us)
    s.set_ref_windows(pq, px, 1, t0=t0)
    out = s._alloc_result(B, 3)
    s._hold(b)
    s._begin(s._options("ms", 3, False, "nonlinear", 0.0, 0.0, 1e10), B, b.x_q, b.x_xi, b.us, None, out)
    s.solve_iterate(3)
    return fields(s.solve_end())


@recipe("windows_schedule", SOLVE + ("tolg_set_weights", "tolg_set_pose_schedule_windows"))
def windows_schedule(make):
    """tolg_set_pose_schedule_windows staged for the next solve.  Bitwise only (as held_schedule)."""
    prob, q, xi, us, pq, px, t0 = _paths()
    s = make(prob)
    s.set_pose_schedule_windows(distinct_schedule(B, 9), 1, t0=t0)
    return fields(s.fit_batch(q, xi, us, **FIT))


@recipe("windows_box", SOLVE + ("tolg_set_al_box_windows", "tolg_set_al"))
def windows_box(make):
    """tolg_set_al_box_windows: the gathered windows are the handle's own torch.empty pair.  Bitwise only: the windows are
    NumPy indexing of the per-knot box, which held_box_knot holds to the oracle."""
    prob, q, xi, us, pq, px, t0 = _paths()
    s = make(prob)
    pl, pu = bx.distinct_box(B, 10, 6, seed=40)
    _, (lam, imu) = mults((B, N_SHORT, 12), 41, s.device, lam=1.0, imu=20.0)
    s.set_al_box_windows(pl, pu, 1, t0=t0, lam=lam, imu=imu)
    out = fields(s.fit_batch(q, xi, us, **FIT))
    s.set_al(None)
    return out


@recipe("windows_obstacles", SOLVE + ("tolg_set_al_obstacle_windows",))
def windows_obstacles(make):
    """tolg_set_al_obstacle_windows.  Bitwise only (as held_spheres_moving)."""
    prob, q, xi, us, pq, px, t0 = _paths()
    s = make(prob)
    path = kd.mixed_slots(pq[..., :3, 3], (0, 0), seed=42, moving=True)
    _, (lam, imu) = mults((B, N_SHORT + 1, 2), 43, s.device)
    s.set_al_obstacle_windows(path, 1, t0=t0, lam=lam, imu=imu)
    out = fields(s.fit_batch(q, xi, us, **FIT))
    s.set_al_obstacles(None)
    return out


@recipe("windows_pose", SOLVE + ("tolg_set_al_pose_constraint_windows",))
def windows_pose(make):
    """tolg_set_al_pose_constraint_windows.  Bitwise only (as held_pose_per_knot)."""
    prob, q, xi, us, pq, px, t0 = _paths()
    s = make(prob)
    path = pk.mixed_slots(pq, pk.MIXED, seed=44, per_knot_form=True)
    _, (lam, imu) = mults((B, N_SHORT + 1, len(pk.MIXED)), 45, s.device)
    s.set_al_pose_constraint_windows(path, 1, t0=t0, kinds=pk.MIXED, lam=lam, imu=imu)
    out = fields(s.fit_batch(q, xi, us, **FIT))
    s.set_al_pose_constraints(None)
    return out


@recipe("held_all_together", SOLVE + ("tolg_set_refs", "tolg_set_weights", "tolg_set_pose_schedule", "tolg_set_al_box", "tolg_set_al",
                                      "tolg_set_al_obstacles_moving", "tolg_set_al_obstacle_kinds", "tolg_set_al_pose_constraints"))
def held_all_together(make):
    """One solve under every held input at once: references, weights and a schedule per trajectory, a box per knot, moving
    slots of every position kind, pose slots per knot.  No single oracle helper states that problem: bitwise only."""
    prob, q, xi, us, q_ref, xi_ref = _multiref()
    Q, P, R = _weights(prob)
    s = make(prob)
    lb, ub = bx.distinct_box(B, N_SHORT, 6, seed=12)
    _, (lam, imu) = mults((B, N_SHORT, 12), 13, s.device, lam=1.0, imu=20.0)
    _, (lam_o, imu_o) = mults((B, N_SHORT + 1, len(kd.CORRIDOR)), 22, s.device)
    _, (lam_p, imu_p) = mults((B, N_SHORT + 1, len(pk.MIXED)), 24, s.device)
    s.set_al(lb, ub, lam, imu)
    s.set_al_obstacles(kd.mixed_slots(q_ref[..., :3, 3], kd.CORRIDOR, seed=21, moving=True), lam_o, imu_o, kinds=kd.CORRIDOR)
    s.set_al_pose_constraints(pk.mixed_slots(q_ref, pk.MIXED, seed=23, per_knot_form=True), pk.MIXED, lam_p, imu_p)
    out = fields(s.fit_batch(q, xi, us, q_ref=q_ref, xi_ref=xi_ref, Q=Q, P=P, R=R, pose_scale=distinct_schedule(B, N_SHORT), **FIT))
    s.set_al_pose_constraints(None)
    s.set_al_obstacles(None)
    s.set_al(None)
    return out


AL_INFO = ("lmbd", "Imu", "mu", "max_violation", "al_converged", "lmbd_obs", "Imu_obs", "lmbd_pose", "Imu_pose")


@recipe("al_fit_everything", SOLVE + ("tolg_set_al_box", "tolg_set_al", "tolg_set_al_obstacles", "tolg_set_al_pose_constraints",
                                      "tolg_al_update_state"))
def al_fit_everything(make):
    """al_fit_batch over two outer iterations under a box per trajectory, spheres and pose cones (tolg_al_update_state).  The
    restated outer loops of the suite take one family each: bitwise only."""
    prob, q, xi, us = _se3()
    s = make(prob)
    lb, ub = (a[:, 0].copy() for a in bx.distinct_box(B, N_SHORT, 6, seed=12, width=0.5))
    res, info = s.al_fit_batch(q, xi, us, lb, ub, n_al_iters=2, n_ilqr_iters=4, tol_constr=1e-12, mu0=1.0,
                               obstacles=_spheres(prob, (0, 0), seed=21), pose_constraints=pk.mixed_slots(_ref_poses(prob), pk.MIXED, seed=23),
                               pose_kinds=pk.MIXED, **TOL0)
    return {**fields(res), **fields(info, "info_", AL_INFO)}


def _al_box_case():
    return _se3()


def _al_box_oracle(make, out):
    """test_al_input_box_at_short_horizons' comparison with al_oracle, at its bounds"""
    prob, q, xi, us0 = _al_box_case()
    box = 0.5 * float(out["free_us"].abs().max())
    lb, ub = -box * np.ones(6), box * np.ones(6)
    for b in range(B):
        o, lam, imu, mu, _ = al_oracle(prob, q[b], xi[b], us0[b], lb, ub, 4, 30, 1e-2)
        assert rel(out["us"][b].cpu(), o["us"]) < 1e-6
        assert rel(out["xs_xi"][b].cpu(), o["xs_xi"]) < 1e-6
        assert rel(out["info_lmbd"][b].cpu(), lam) < 1e-6
        assert abs(float(out["info_mu"][b]) / mu - 1) < 1e-6  # (pytest.approx's default)
        np.testing.assert_array_equal(out["info_Imu"][b].cpu().numpy() == 0.0, imu == 0.0)


@recipe("al_fit_shared_box", SOLVE + ("tolg_set_al", "tolg_al_update"), _al_box_oracle)
def al_fit_shared_box(make):
    """al_fit_batch under one shared box (tolg_al_update) at half the unconstrained solution's largest input, the case of
    test_al_input_box_at_short_horizons at B = 5, against the restated outer loop (al_oracle)."""
    prob, q, xi, us0 = _al_box_case()
    s = make(prob)
    free = s.fit_batch(q, xi, us0, mode="ms", n_iterations=30)
    box = 0.5 * float(free.us.abs().max())
    res, info = s.al_fit_batch(q, xi, us0, -box * np.ones(6), box * np.ones(6), n_al_iters=4, n_ilqr_iters=30, tol_constr=1e-2)
    return {"free_us": free.us, **fields(res), **fields(info, "info_", AL_INFO)}


# ---- the outer update of a constrained MPC step, as a single call ---------------------------------------------------------
STEP = dict(mu0=0.5, mu_scale=10.0, mu_max=1e8, tol=1e-2, Ks=2, Kp=3, seed=77)
STEP_RT, STEP_AT = 1e-12, 1e-15  # test_step_against_the_restatement's (tests/test_gpu_mpc_constrained.py, tests/test_gpu_pose_mpc.py)


def _step_case():
    """tests/pose_mpc.py::step_case on the short se3 problem's N and m: a shared box, static spheres and static pose slots, g of
    both signs in every family, the last trajectory satisfying everything (it holds mu beside the violating ones)."""
    from tests import pose_mpc as pm
    return pm, pm.step_case(N_SHORT, 6, B, STEP["Ks"], STEP["Kp"], "box+static+pose", [B - 1], STEP["seed"])


def _step_oracle(make, out):
    """al_mpc_step_restated (tests/mpc_al.py, with g_box and g_spheres) for the box with spheres, al_mpc_step_restated3
    (tests/pose_mpc.py) with the pose rows beside them, on the returned tensors themselves, at the bounds and under the
    preconditions of the two test_step_against_the_restatement: max_violation and lambda' to rtol 1e-12 / atol 1e-15, mu and
    I_mu' exactly."""
    pm, c = _step_case()
    rows = pm.step_rows(c)
    assert np.array_equal(rows[0][0], g_box(c["us"], c["lb"], c["ub"])) and np.array_equal(rows[1][0], g_spheres(c["xs_q"], c["obs"]))
    assert pm.clear_of_branch_points(rows) > pm.CLEAR and pm.lambda_error_bound(c, rows) < 1.0
    for r in rows:
        assert (r[0][:B - 1] > STEP["tol"]).any() and (r[0][:B - 1] < 0).any()
    mu0 = np.full(B, STEP["mu0"])
    for shift in (0, 1):
        for name, want in (("spheres", al_mpc_step_restated(mu0, STEP["mu_scale"], STEP["mu_max"], STEP["tol"], shift, rows[0], rows[1])),
                           ("pose", pm.al_mpc_step_restated3(mu0, STEP["mu_scale"], STEP["mu_max"], STEP["tol"], shift, *rows))):
            key = "%s_shift%d_" % (name, shift)
            assert np.allclose(host(out[key + "maxviol"]), want[0], rtol=STEP_RT, atol=STEP_AT), key
            assert np.array_equal(host(out[key + "mu"]), want[1]), key
            assert np.array_equal(host(out[key + "mu"]), np.where(np.arange(B) == B - 1, STEP["mu0"], 10 * STEP["mu0"])), key
            for fam, e in zip(("box", "sph", "pose"), want[2:]):
                assert np.allclose(host(out[key + fam + "_lam"]), e[0], rtol=STEP_RT, atol=STEP_AT), (key, fam)
                assert np.array_equal(host(out[key + fam + "_imu"]), e[1]), (key, fam)


@recipe("al_mpc_step", ("tolg_al_mpc_step", "tolg_al_mpc_step_pose", "tolg_set_al", "tolg_set_al_obstacles",
                        "tolg_set_al_pose_constraints"), _step_oracle)
def al_mpc_step(make):
    """tolg_al_mpc_step (a box with spheres) and tolg_al_mpc_step_pose (a box with spheres and pose slots) as single calls on
    a handle that has done nothing else, with and without the shift: max_violation, mu and the multipliers each call updates in
    place, against the restatements of tests/mpc_al.py and tests/pose_mpc.py."""
    pm, c = _step_case()
    prob = _se3()[0]
    out = {}
    for name in ("spheres", "pose"):
        for shift in (0, 1):
            s = make(prob)
            dev = s.device
            m = {fam: [f64(a, dev) for a in c[fam]] for fam in ("box", "sph", "pose")}
            s.set_al(c["lb"], c["ub"], *m["box"])
            s.set_al_obstacles(c["obs"], *m["sph"])
            if name == "pose":
                s.set_al_pose_constraints(c["slots"], c["kinds"], *m["pose"])
            mu = torch.full((B,), STEP["mu0"], dtype=torch.float64, device=dev)
            mv = s.al_mpc_step(f64(c["xs_q"], dev), f64(c["us"], dev), mu, STEP["mu_scale"], STEP["mu_max"], STEP["tol"], bool(shift))
            torch.cuda.synchronize()
            s.set_al_pose_constraints(None)
            s.set_al_obstacles(None)
            s.set_al(None)
            key = "%s_shift%d_" % (name, shift)
            out.update({key + "maxviol": mv, key + "mu": mu})
            for fam in ("box", "sph") + (("pose",) if name == "pose" else ()):
                out.update({key + fam + "_lam": m[fam][0], key + fam + "_imu": m[fam][1]})
    return out


# ---- the held policy --------------------------------------------------------------------------------------------------------
def _pert():
    return pert(B, S, N_SHORT, seed=11)


def _restatement_oracle(make, out):
    prob, s, r, *_ = _held(make)
    check_restatement(s, r, [op_of(prob)] * B, *_pert())


@recipe("policy_rollout", SOLVE + ("tolg_policy_rollout", "tolg_solve_gains"), _restatement_oracle)
def policy_rollout(make):
    """tolg_policy_rollout with trajectories; check_restatement on a handle of its own."""
    prob, s, r, *_ = _held(make)
    return tensors(s.policy_rollout(*_pert(), trajectories=True))


def _nominal(r):
    return Nominal(host(r.xs_q), host(r.xs_xi), host(r.us))


def _limited_box(prob, s, r, dx0, w):
    return restate_limited_batch([op_of(prob)] * B, _nominal(r), host(s.gains()["K"]), dx0, w)


@recipe("policy_rollout_limited", SOLVE + ("tolg_policy_rollout_limited", "tolg_solve_gains"))
def policy_rollout_limited(make, check=False):
    """tolg_policy_rollout_limited under the box of tests/limits.py (from the unlimited restatement); with check, compare_limited
    against restate_policy_limited at its bounds."""
    prob, s, r, *_ = _held(make)
    dx0, w = _pert()
    lb, ub, R = _limited_box(prob, s, r, dx0, w)
    p = s.policy_rollout(dx0, w, trajectories=True, u_lb=lb, u_ub=ub)
    if check:
        fin = np.array([np.isfinite(x["J"]) for x in R])
        near = np.array([near_bound(x["uc"], lb[b], ub[b]) for b, x in enumerate(R)]) & fin
        compare_limited(p, R, fin, near)
    return tensors(p)


policy_rollout_limited.oracle = lambda make, out: policy_rollout_limited(make, check=True)


@recipe("policy_rollout_margins", SOLVE + ("tolg_policy_rollout_margins", "tolg_set_al_obstacles", "tolg_set_al_obstacle_kinds",
                                           "tolg_set_al_pose_constraints"))
def policy_rollout_margins(make):
    """tolg_policy_rollout_margins: clearance, pose margin and per-knot counts under five slots of each family on the nominal
    (tests/margins.py), beside a box.  Its reference is rollout_margins on returned trajectories, a property of the outputs, not
    an oracle: bitwise only."""
    prob, s, r, *_ = _held(make)
    xq = host(r.xs_q)
    s.set_al_obstacles(mg.position_slots(xq, mg.OBS_KINDS[5]), kinds=mg.OBS_KINDS[5])
    s.set_al_pose_constraints(mg.pose_slots(xq, mg.POSE_KINDS[5], per_knot=True), mg.POSE_KINDS[5])
    u = float(r.us.abs().max())
    p = s.policy_rollout(*_pert(), trajectories=True, u_lb=-0.8 * u * np.ones(6), u_ub=0.8 * u * np.ones(6), clearance=True,
                         pose_margin=True, violations=True)
    s.set_al_pose_constraints(None)
    s.set_al_obstacles(None)
    return tensors(p)


def _actuator(r):
    u = host(r.us)
    return dict(u_lb=u.min(axis=1) - 0.05, u_ub=u.max(axis=1) + 0.05, act_tau=np.full(6, 0.1), act_rate=np.full(6, 4.0))


def _actuated_recipe(delay):
    def run(make, check=False):
        prob, s, r, *_ = _held(make)
        dx0, w = _pert()
        a = _actuator(r)
        p = s.policy_rollout(dx0, w, trajectories=True, commands=True, act_delay=delay, **a)
        if check:
            from trajectory_optimization_matrix_lie_groups_amd import check_actuator
            lb, ub, beta, du, _, _ = check_actuator(a["u_lb"], a["u_ub"], a["act_tau"], a["act_rate"], delay, None, B, 6, prob.dt)
            nom, K, op = _nominal(r), host(s.gains()["K"]), op_of(prob)
            for b in range(B):
                R = restate_policy_actuated(op, nom.xs_q[b], nom.xs_xi[b], nom.us[b], K[b], lb[b], ub[b], beta[b], du[b], delay, None,
                                            dx0[b], w[b], S)
                fin = np.isfinite(R["J"])
                assert np.array_equal(host(p.status)[b], np.where(fin, _capi.ST_OK, _capi.ST_NONFINITE))
                # check_restatement's bounds
                assert np.abs(host(p.xs_q)[b][fin] - R["xs_q"][fin]).max(initial=0) < 1e-10
                assert np.abs(host(p.xs_xi)[b][fin] - R["xs_xi"][fin]).max(initial=0) < 1e-10
                assert np.abs(host(p.us)[b][fin] - R["us"][fin]).max(initial=0) < 1e-8
                assert np.abs(host(p.u_cmd)[b][fin] - R["uc"][fin]).max(initial=0) < 1e-8
                assert np.abs(host(p.J)[b][fin] / R["J"][fin] - 1).max(initial=0) < 1e-9
        return tensors(p)

    run.__doc__ = ("tolg_policy_rollout_actuated with a box, a lag, a rate limit and a delay of %d knots (the delay ring in LDS); the "
                   "check is restate_policy_actuated at check_restatement's bounds." % delay)
    run = recipe("policy_rollout_actuated_d%d" % delay, SOLVE + ("tolg_policy_rollout_actuated", "tolg_solve_gains"))(run)
    run.oracle = lambda make, out: run(make, check=True)


_actuated_recipe(0)
_actuated_recipe(4)


def _estimated_inputs(prob):
    rng = np.random.default_rng(5)
    dx0, w = _pert()
    n = rng.normal(size=(B, S, N_SHORT + 1, 12)) * 0.01
    return dx0, w, n, psd(B, 12, 0.05, 7), psd(B, 6, 0.01, 8), np.full((B, 12), 1e-3)


def _estimated_recipe(limited):
    def run(make, check=False):
        prob, s, r, *_ = _held(make)
        dx0, w, n, S0, W, V = _estimated_inputs(prob)
        c = s.policy_covariance_estimated(S0, W, 0xFFF, V, gains=True)
        kw = {}
        if limited:
            u = host(r.us)
            kw = dict(u_lb=u.min(axis=1) - 0.05, u_ub=u.max(axis=1) + 0.05)
        p = s.policy_rollout_estimated(c.L, 0xFFF, dx0, w, n, trajectories=True, estimates=True, **kw)
        if check and not limited:
            nom, K, L, op = _nominal(r), host(s.gains()["K"]), host(c.L), op_of(prob)
            R = []
            for b in range(B):
                J, xq, xx, uu, eq, ex = restate_rollout_estimated(op, nom.xs_q[b], nom.xs_xi[b], nom.us[b], K[b], L[b], 0xFFF, dx0[b],
                                                                   w[b], n[b], S)
                R.append(dict(J=J, xs_q=xq, xs_xi=xx, us=uu, est_q=eq, est_xi=ex))
            compare_estimated(p, R, np.ones((B, S), bool))
        return {**tensors(p), "L": c.L}

    run.__doc__ = ("tolg_policy_rollout_estimated%s on the gains of tolg_policy_covariance_estimated, every coordinate measured.  %s"
                   % ("_limited" if limited else "", "The limited form has no restatement helper: bitwise only." if limited else
                      "compare_estimated against restate_rollout_estimated."))
    run = recipe("policy_rollout_estimated" + ("_limited" if limited else ""),
                 SOLVE + ("tolg_policy_covariance_estimated", "tolg_solve_gains",
                          "tolg_policy_rollout_estimated_limited" if limited else "tolg_policy_rollout_estimated"))(run)
    if not limited:
        run.oracle = lambda make, out: run(make, check=True)


_estimated_recipe(False)
_estimated_recipe(True)


@recipe("policy_covariance", SOLVE + ("tolg_policy_covariance", "tolg_policy_covariance_estimated"))
def policy_covariance(make):
    """tolg_policy_covariance and its estimated form, with and without Sigma (full) and with neither moment (se3; the drone's
    m = 4 with the moments).  Their restatements (tests/restate.py, tests/estimated.py) are not assertion-bearing helpers:
    bitwise only."""
    out = {}
    for name in ("se3", "drone"):
        prob, s, r, *_ = _held(make, name)
        S0, W, V = psd(B, 12, 0.05, 7), psd(B, 6, 0.01, 8), np.full((B, 12), 1e-3)
        out.update(tensors(s.policy_covariance(S0, W, full=True), name + "_full_"))
        out.update(tensors(s.policy_covariance(S0, W), name + "_diag_"))
        out.update(tensors(s.policy_covariance(), name + "_zero_"))
        out.update(tensors(s.policy_covariance_estimated(S0, W, 0x03F, V, full=True, gains=True), name + "_est_full_"))
        out.update(tensors(s.policy_covariance_estimated(S0, W, 0xFFF, V), name + "_est_diag_"))
    return out


@recipe("policy_value", SOLVE + ("tolg_policy_value", "tolg_set_refs", "tolg_set_weights"))
def policy_value(make):
    """tolg_policy_value with and without P (full), on the shared problem and on per-trajectory references and weights.
    Bitwise only (as policy_covariance)."""
    prob, s, r, *_ = _held(make)
    S0, W = psd(B, 12, 0.05, 7), psd(B, 6, 0.01, 8)
    out = {**tensors(s.policy_value(S0, W, full=True), "full_"), **tensors(s.policy_value(), "plain_")}
    prob, q, xi, us, q_ref, xi_ref = _multiref()
    Q, P, R = _weights(prob)
    s = make(prob)
    s.fit_batch(q, xi, us, q_ref=q_ref, xi_ref=xi_ref, Q=Q, P=P, R=R, **FIT)
    out.update(tensors(s.policy_value(S0, W, full=True), "pt_"))
    return out


@recipe("policy_rollout_plant", SOLVE + ("tolg_set_plant", "tolg_policy_rollout"))
def policy_rollout_plant(make):
    """tolg_set_plant: a plant per sample (dense inertia blocks) and one per trajectory (diagonal) under tolg_policy_rollout.
    restate_plant_policy is not an assertion-bearing helper: bitwise only."""
    prob, s, r, *_ = _held(make)
    dx0, w = _pert()
    dense = workloads.plant_mismatch(B, S, N=N_SHORT, rotate=True, seed=2)[6]
    diag = workloads.plant_mismatch(B, 1, N=N_SHORT, seed=3)[6][:, 0]
    return {**tensors(s.policy_rollout(dx0, w, trajectories=True, plant_J=dense), "dense_"),
            **tensors(s.policy_rollout(dx0, w, trajectories=True, plant_J=diag), "diag_")}


# ---- MPC ----------------------------------------------------------------------------------------------------------------
MPC_STEPS = 3
MPC = ("tolg_set_ref_windows", "tolg_solve_begin", "tolg_solve_begin_warm", "tolg_solve_iterate", "tolg_solve_end")
MPC_FIELDS = ("xs_q", "xs_xi", "us", "J", "iters", "status", "n_sat", "n_rate", "max_violation", "mu", "clearance", "pose_margin",
              "est_q", "est_xi", "est_var", "innov")


def _mpc_case(**kw):
    return workloads.se3_mpc(B, MPC_STEPS, N=N_SHORT, sigma_noise=0.02, seed=21, **kw)


def _mpc_kw(t0, noise, **kw):
    return dict(t0=t0, first_iters=6, iters_per_step=3, noise=noise, check_every=0, **TOL0, **kw)


@recipe("mpc_plain", MPC + ("tolg_mpc_advance",), lambda make, out: check_loop(B=B, N=N_SHORT, steps=MPC_STEPS, K0=6, K=3))
def mpc_plain(make):
    """mpc() for three steps, warm-started in states and in controls; check_loop (its own handle, B = 5) against
    restate_mpc_step."""
    prob, q, xi, pq, px, t0, noise = _mpc_case()
    out = fields(make(prob).mpc(q, xi, pq, px, MPC_STEPS, warm="states", **_mpc_kw(t0, noise)), "states_", MPC_FIELDS)
    out.update(fields(make(prob).mpc(q, xi, pq, px, MPC_STEPS, warm="controls", **_mpc_kw(t0, noise)), "controls_", MPC_FIELDS))
    return out


@recipe("mpc_constrained", MPC + ("tolg_mpc_advance", "tolg_set_al_box", "tolg_set_al", "tolg_set_al_obstacle_windows",
                                  "tolg_set_al_pose_constraints", "tolg_al_mpc_step_pose", "tolg_al_mpc_step", "tolg_set_al_box_windows",
                                  "tolg_set_al_obstacles"))
def mpc_constrained(make):
    """mpc() under a box per knot, one moving sphere and one tilt cone (tolg_al_mpc_step_pose), and on a second handle under a
    world-time box and a static sphere (tolg_al_mpc_step).  The step itself is held to its restatement in the al_mpc_step
    recipe; the suite has no helper that restates the constrained loop as a whole: bitwise only."""
    prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, MPC_STEPS, N=N_SHORT, K=1, sigma_noise=0.02, seed=21)
    lb, ub = bx.distinct_box(B, N_SHORT, 6, seed=12, width=5.0)
    tilt = np.array([[0.0, 0.0, 1.0, 0.2]])
    kw = _mpc_kw(t0, noise, first_al_iters=2, al_iters_per_step=1, mu0=1.0)
    out = fields(make(prob).mpc(q, xi, pq, px, MPC_STEPS, lb=lb, ub=ub, obstacle_paths=mov, pose_constraints=tilt,
                                pose_kinds=(pk.TILT,), **kw), "pose_", MPC_FIELDS)
    pl, pu = bx.distinct_box(B, pq.shape[1], 6, seed=40, width=5.0)
    out.update(fields(make(prob).mpc(q, xi, pq, px, MPC_STEPS, lb_path=pl, ub_path=pu, obstacles=obs, **kw), "path_", MPC_FIELDS))
    return out


@recipe("mpc_actuated", MPC + ("tolg_mpc_advance_actuated",))
def mpc_actuated(make):
    """mpc() behind an actuator with a lag, a rate limit and a delay of two knots: the loop's own act_state is a torch.empty it
    fills behind the first solve.  tests/test_gpu_actuator.py holds it to a host loop of restated steps; no helper: bitwise only."""
    prob, q, xi, pq, px, t0, noise = _mpc_case()
    r = make(prob).mpc(q, xi, pq, px, MPC_STEPS, warm="controls", act_tau=np.full(6, 0.1), act_rate=np.full(6, 4.0), act_delay=2,
                       **_mpc_kw(t0, noise))
    return fields(r, "", MPC_FIELDS)


@recipe("mpc_estimated", MPC + ("tolg_mpc_measure", "tolg_mpc_advance_estimated", "tolg_set_plant"))
def mpc_estimated(make):
    """mpc() on a Kalman filter's estimate, without and with a plant (and the actuator's box).  restate_mpc_estimated
    (tests/mpc_estimated.py) is compared in tests/test_gpu_mpc_estimated.py with bounds of its own; no helper: bitwise only."""
    prob, q, xi, pq, px, t0, noise, est = workloads.se3_mpc_estimated(B, MPC_STEPS, N=N_SHORT, sigma_noise=0.02, seed=21)
    kw = _mpc_kw(t0, noise, meas_mask=0xFFF, **est)
    out = fields(make(prob).mpc(q, xi, pq, px, MPC_STEPS, warm="controls", **kw), "model_", MPC_FIELDS)
    PJ = workloads.plant_mismatch(B, 1, N=N_SHORT, sigma_inertia=0.2, seed=2)[6][:, 0]
    kw["meas_mask"] = 0x03F
    out.update(fields(make(prob).mpc(q, xi, pq, px, MPC_STEPS, warm="states", plant_J=PJ, u_lb=-5.0 * np.ones(6), u_ub=5.0 * np.ones(6),
                                     **kw), "plant_", MPC_FIELDS))
    return out


ADVANCE = ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us", "J_cl", "n_sat", "n_rate")


def _advance_oracle(make, out):
    prob, s, r, *_ = _held(make)
    check_advance(s, r, [op_of(prob)] * B, np.random.default_rng(3).normal(0, 0.01, (B, 6)))


@recipe("mpc_advance_forms", SOLVE + ("tolg_mpc_advance", "tolg_mpc_advance_limited", "tolg_mpc_advance_actuated", "tolg_set_plant"),
        _advance_oracle)
def mpc_advance_forms(make):
    """The single-step calls on one held policy: tolg_mpc_advance plain and on a plant, tolg_mpc_advance_limited,
    tolg_mpc_advance_actuated (delay 2, its state from actuator_state).  check_advance on a handle of its own covers the plain
    form; the others have restatements without an assertion-bearing helper."""
    prob, s, r, *_ = _held(make)
    wa = np.random.default_rng(3).normal(0, 0.01, (B, 6))
    u0 = host(r.us)[:, 0]
    J = [torch.zeros(B, dtype=torch.float64, device=s.device) for _ in range(4)]
    out = fields(s.mpc_advance(wa, J_cl=J[0]), "plain_", ADVANCE)
    PJ = workloads.plant_mismatch(B, 1, N=N_SHORT, sigma_inertia=0.2, seed=2)[6][:, 0]
    out.update(fields(s.mpc_advance(wa, J_cl=J[1], plant_J=PJ), "plant_", ADVANCE))
    out.update(fields(s.mpc_advance(wa, J_cl=J[2], u_lb=u0 - 0.01, u_ub=u0 + 0.02), "limited_", ADVANCE))
    st = actuator_state(r.us[:, 0] + 0.1, 2)
    out.update(fields(s.mpc_advance(wa, J_cl=J[3], u_lb=u0 - 0.01, u_ub=u0 + 0.02, act_tau=0.1, act_rate=4.0, act_delay=2,
                                    act_state=st), "actuated_", ADVANCE))
    out["act_state"] = st
    return out


def _measure_inputs():
    prob, q, xi, us = _model("se3", B, N_SHORT)
    rng = np.random.default_rng(9)
    eq = np.array([q[b] @ ob.se3_exp(rng.normal(size=6) * 0.02) for b in range(B)])
    return prob, q, xi, us, eq, xi + rng.normal(size=(B, 6)) * 0.02, psd(B, 12, 0.02, 7), np.full((B, 12), 1e-4), rng.normal(size=(B, 12)) * 0.01


def _measure_oracle(make, out):
    """restate_measure (tests/mpc_estimated.py) at test_gpu_mpc_estimated's bounds for the measure: 1e-10 absolute on the estimate
    (check_restatement's state bound), 1e-9 relative on P, L and the innovation"""
    prob, q, xi, us, eq, exi, P, V, n = _measure_inputs()
    for b in range(B):
        m = restate_measure(q[b], xi[b], eq[b], exi[b], P[b], 0xFFF, V[b], n[b])
        assert np.abs(host(out["est_q"])[b].reshape(4, 4) - m["est_q"]).max() < 1e-10
        assert np.abs(host(out["est_xi"])[b] - m["est_xi"]).max() < 1e-10
        assert rel(host(out["P"])[b], m["P"]) < 1e-9 and rel(host(out["L"])[b], m["L"]) < 1e-9
        assert rel(host(out["innov"])[b], m["innov"]) < 1e-9 and rel(host(out["var_est"])[b], m["var_est"]) < 1e-9


@recipe("mpc_measure", ("tolg_mpc_measure",), _measure_oracle)
def mpc_measure(make):
    """tolg_mpc_measure as the first call on its handle (it needs no held policy), against restate_measure."""
    prob, q, xi, us, eq, exi, P, V, n = _measure_inputs()
    s = make(prob)
    d = [f64(a, s.device) for a in (q.reshape(B, 16), xi, eq.reshape(B, 16), exi, P)]
    r = s.mpc_measure(0xFFF, V, *d, noise=n)
    return {**tensors(r), "est_q": d[2], "est_xi": d[3], "P": d[4]}


@recipe("mpc_advance_estimated", SOLVE + ("tolg_mpc_advance_estimated",))
def mpc_advance_estimated(make):
    """tolg_mpc_advance_estimated on a held policy, with the box and W.  restate_advance_estimated has no assertion-bearing
    helper: bitwise only."""
    prob, s, r, q, xi, us = _held(make)
    rng = np.random.default_rng(4)
    tq = f64(np.array([q[b] @ ob.se3_exp(rng.normal(size=6) * 0.02) for b in range(B)]).reshape(B, 16), s.device)
    txi, P = f64(xi + rng.normal(size=(B, 6)) * 0.02, s.device), f64(psd(B, 12, 0.02, 7), s.device)
    u0 = host(r.us)[:, 0]
    J = torch.zeros(B, dtype=torch.float64, device=s.device)
    a = s.mpc_advance_estimated(tq, txi, P, w=rng.normal(0, 0.01, (B, 6)), W=psd(B, 6, 0.01, 8), J_cl=J, u_lb=u0 - 0.01, u_ub=u0 + 0.02)
    return {**fields(a, "", ADVANCE), "x_true_q": tq, "x_true_xi": txi, "P": P}


NAMES = [r.name for r in RECIPES]
# the entry points no recipe has to reach: they launch nothing on a handle's workspace
EXEMPT = ("tolg_destroy", "tolg_workspace_bytes", "tolg_refs_bytes", "tolg_weights_bytes", "tolg_pose_schedule_bytes",
          "tolg_obstacles_bytes", "tolg_obstacles_moving_bytes", "tolg_pose_constraints_bytes", "tolg_plant_bytes",
          "tolg_kernel_time", "tolg_enable_timing", "tolg_selftest_series")


def run_recipe(fn, pattern):
    """One recipe under one pattern: the tensors it returns, the device idle behind them."""
    from tests.poison import poisoned
    with poisoned(pattern):
        out = fn(make_solver)
        torch.cuda.synchronize()
    return out


def as_bits(out):
    """{name: integer numpy array of the tensor's bytes}: float64 as int64, the integer types as they are"""
    res = {}
    for k, v in out.items():
        v = v.detach().contiguous()
        res[k] = (v.view(torch.int64) if v.dtype == torch.float64 else v).cpu().numpy()
    return res


def run_table_to_npz(path, pattern):
    """The body of the TOLG_POISON_LDS child process: every recipe once under `pattern`, every tensor's bits into one .npz
    under "<recipe>/<tensor>"."""
    blob = {}
    for fn in RECIPES:
        for k, v in as_bits(run_recipe(fn, pattern)).items():
            blob["%s/%s" % (fn.name, k)] = v
    np.savez(path, **blob)
