#!/usr/bin/env python3
"""Randomised parity sweep on the GPU: the instantiation matrix of tests/test_gpu_matrix.py with everything drawn at random
(model kind, inertia structure, solver mode, line search, rollout form, batch, horizon, weights over four decades, time
step, the spread of the initial states and of the initial controls), each case against the oracle.  Looks for the rare
paths the fixed cases do not visit (regularisation retries, the max-regularisation exit, the closed-form tiers of the
series, deep backtracking).  Prints one line per disagreement with the seed that reproduces it.
    python tools/parity_fuzz.py [--large | --edge] [cases] [first seed]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bridge as ob  # noqa: E402  (test infrastructure: the checker)
from oracle import bridge_ld as obl  # noqa: E402  (its long-double twin: the referee)
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, workloads  # noqa: E402

TOL_J = 1e-9     # relative, per iteration -- or ten times what the fp64 oracle itself is away from its long-double twin at that
                 # iteration (oracle/tolg_oracle_ld.c: the same statements with 11 more mantissa bits), whichever is larger.  Round 3
                 # widened this number to 1e-8 after seeds 2352 and 30037; both are problems that amplify the last bit of anything
                 # (profiles/r04_parity_referee.txt: the fp64 ORACLE is 7e-9 resp. 2.2e-8 from the long-double evaluation there)
TOL_U = 1e-6     # controls at the end of the solve (north_star's figure) for problems with R >= 1e-4 ...
TOL_U_FLAT = 1e-5  # ... and for the draws with an input weight below that, where the cost is nearly flat in u (seed 7230: controls
                 # 1.3e-6 apart under costs that agree to 1e-13); the referee's distance widens both in the same way
REFEREE = True   # --no-referee: fixed tolerances only


LARGE = False    # --large: batches of 500 .. 6 000 (the compacted lists and the thread form of the wide line-search stages,
                 # many workgroups, padded tails), horizons of 40 .. 200


NKINDS = 5       # model kinds drawn from: the first campaign (seeds 1000 .. 6999) drew among the first three, the second among four


EDGE_BATCHES = (1, 2, 3, 4, 15, 16, 17, 20, 63, 64, 65, 68)   # shapes="edge": padded lanes, short last workgroups, the 64-wide grids


def draw(seed, nkinds=None, shapes="default"):
    """One random case: (cfg, prob or (prob, oracle problem), x0_q, x0_xi, us0).  shapes="edge" draws the horizon from
    [1, 34) (every branch of the short-horizon rings and pipelines) and the batch from EDGE_BATCHES instead; every other
    draw, and the default draws themselves, stay as they are."""
    rng = np.random.default_rng(seed)
    kind = ["se3", "rigidbody", "drone", "so3", "pendulum"][rng.integers(nkinds or NKINDS)]
    diag = bool(rng.integers(4) > 0)
    mode = ["ms", "ss"][rng.integers(2)]
    line_search = bool(rng.integers(2)) if mode == "ms" else False
    rollout = ["nonlinear", "linear"][int(rng.integers(4) == 0)]
    if shapes == "edge":
        B, N = EDGE_BATCHES[int(rng.integers(len(EDGE_BATCHES)))], int(rng.integers(1, 34))
    else:
        B, N = int(rng.integers(1, 10)), int(rng.integers(3, 70))
    if LARGE:
        B, N = int(rng.integers(500, 6000)), int(rng.integers(40, 201))
    if kind == "pendulum":
        # Pendulum3dDyanmics (state-dependent F_u block, the sweep's first form with per-knot input matrices) on the stored
        # swing-up path: random inertia, mass, length, weights; horizon = the path's 80 knots or a prefix of it
        from trajectory_optimization_matrix_lie_groups_amd.solver import embed_pendulum3d
        base, x0_q, x0_xi, _ = workloads.pendulum_swingup(B, xi0_scale=float(rng.uniform(0.5, 5.0)), seed=seed)
        N = min(N, base.N) if not LARGE else base.N
        J3 = np.diag(rng.uniform(0.3, 1.5, 3))
        mass, length = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.2, 1.0))
        Q6, P6, R3 = np.diag(10.0 ** rng.uniform(-1, 2, 6)), np.diag(10.0 ** rng.uniform(-1, 3, 6)), np.diag(10.0 ** rng.uniform(-4, -1, 3))
        R_ref, w_ref = base.q_ref[: N + 1, :3, :3], base.xi_ref[: N + 1, :3]
        prob = embed_pendulum3d(J3, mass, length, base.dt, Q6, R3, P6, R_ref, w_ref)
        us0 = np.zeros((B, N, 6)); us0[..., :3] = rng.normal(size=(B, N, 3)) * 10.0 ** rng.uniform(-3, -0.5)
        K = int(rng.integers(3, 14)) if not LARGE else int(rng.integers(3, 8))
        cfg = dict(kind=kind, diag=True, mode=mode, line_search=line_search, rollout=rollout, B=B, N=N, K=K)
        return cfg, (prob, ob.embed_pendulum_problem(J3, mass, length, base.dt, Q6, R3, P6, R_ref, w_ref)), x0_q, x0_xi, us0
    if kind == "so3":
        # SO3Dynamics + the SO3 tracking cost (terminal l / l_x with Q, App. C-Q3: P is drawn independently of Q) in the
        # SE(3) containers: translation, linear velocity and inputs 3..5 identically zero
        from trajectory_optimization_matrix_lie_groups_amd.solver import embed_so3
        base, x0_q, x0_xi, _ = workloads.so3_tracking(B, N=N, seed=seed)
        J3 = np.diag(rng.uniform(0.3, 2.0, 3))
        Q6, P6, R3 = np.diag(10.0 ** rng.uniform(-1, 2, 6)), np.diag(10.0 ** rng.uniform(-1, 3, 6)), np.diag(10.0 ** rng.uniform(-6, -2, 3))
        dt = float(base.dt * rng.uniform(0.6, 1.5))
        R_ref, w_ref = base.q_ref[:, :3, :3], base.xi_ref[:, :3]
        prob = embed_so3(J3, dt, Q6, R3, P6, R_ref, w_ref)
        us0 = np.zeros((B, N, 6)); us0[..., :3] = rng.normal(size=(B, N, 3)) * 10.0 ** rng.uniform(-3, -0.5 if not LARGE else -1.5)
        x0_xi = x0_xi.copy(); x0_xi[:, :3] += rng.normal(size=(B, 3)) * 10.0 ** rng.uniform(-2, -0.3)
        K = int(rng.integers(3, 14)) if not LARGE else int(rng.integers(3, 8))
        cfg = dict(kind=kind, diag=True, mode=mode, line_search=line_search, rollout=rollout, B=B, N=N, K=K)
        return cfg, (prob, ob.embed_so3_problem(J3, dt, Q6, R3, P6, R_ref, w_ref)), x0_q, x0_xi, us0
    base, x0_q, x0_xi, _ = (workloads.drone_tracking if kind == "drone" else workloads.se3_tracking)(B, N=N, seed=seed)
    m = 4 if kind == "drone" else 6
    J = np.diag(rng.uniform(0.3, 2.0, 6))
    if not diag:
        A = rng.normal(size=(3, 3)) * 0.15
        J[:3, :3] += A @ A.T
        A = rng.normal(size=(3, 3)) * 0.1
        J[3:, 3:] = np.eye(3) * rng.uniform(0.8, 1.4) + (0 if kind in ("drone", "rigidbody") else A @ A.T)
    if kind in ("drone", "rigidbody"):
        J[3:, 3:] = np.eye(3) * J[4, 4] if diag else J[3:, 3:]
    Q = np.diag(10.0 ** rng.uniform(-1, 2, 12))
    R = np.diag(10.0 ** rng.uniform(-6, -2, m))
    if not diag:
        Bm = rng.normal(size=(m, m)) * 1e-3
        R = R + Bm @ Bm.T
    dt = float(base.dt * rng.uniform(0.6, 1.5))
    prob = TrackingProblem(kind, J, dt, Q, R, rng.uniform(1.0, 10.0) * Q, base.q_ref, base.xi_ref)
    us0 = rng.normal(size=(B, N, m)) * 10.0 ** rng.uniform(-3, -0.5 if not LARGE else -1.5)
    x0_xi = x0_xi + rng.normal(size=x0_xi.shape) * 10.0 ** rng.uniform(-2, -0.3)
    K = int(rng.integers(3, 14)) if not LARGE else int(rng.integers(3, 8))
    return dict(kind=kind, diag=diag, mode=mode, line_search=line_search, rollout=rollout, B=B, N=N, K=K), prob, x0_q, x0_xi, us0


_PD_CACHE = {}


def pd_flip(b, solver, op, cfg, x0_q, x0_xi, us0, st, o, mu_g, mu_o, Jg):
    """One side of trajectory b ran clean, the other regularised to the limit / went non-finite.  Give the clean side the failing
    side's trajectory at the sweep where the two part (k = first iteration whose regularisation differs) and run ITS backward pass
    on it: True if it then regularises past max_reg as well -- the decision belongs to the trajectory's last digits, not to the
    implementation."""
    n = min(len(mu_g), len(mu_o))
    ks = [k for k in range(n) if (mu_g[k] > 0) != (mu_o[k] > 0) or not np.isfinite(Jg[b, k]) or not np.isfinite(o["J_hist"][b, k])]
    if not ks:
        return False
    k, ms = ks[0], cfg["mode"] == "ms"
    kw = dict(mode=cfg["mode"], line_search=cfg["line_search"], rollout=cfg["rollout"])
    try:
        if o["status"][b] == 0:   # the GPU failed: the oracle's sweep on the GPU's trajectory
            key = ("g", id(solver), k)
            if key not in _PD_CACHE:
                _PD_CACHE.clear()
                if k == 0:
                    _PD_CACHE[key] = None
                else:
                    rk = solver.fit_batch(x0_q, x0_xi, us0, n_iterations=k, tol_grad_norm=0.0, tol_d_norm=0.0, **kw)
                    _PD_CACHE[key] = (rk.xs_q.cpu().numpy(), rk.xs_xi.cpu().numpy(), rk.us.cpu().numpy())
            if _PD_CACHE[key] is None:
                return False
            xq, xx, uu = _PD_CACHE[key]
            lb = ob.lin_backward(op, xq[b], xx[b], uu[b], ms=ms, mu=0.0)
            return bool(lb["mu"] >= 1e10 or not np.isfinite(lb["grad"]))
        # the oracle failed: the GPU's sweep on the oracle's trajectory
        if k == 0:
            return False
        ok_ = ob.fit_batch(op, x0_q, x0_xi, us0, max_iter=k, **kw)
        g = solver.linearize_backward(ok_["xs_q"], ok_["xs_xi"], ok_["us"], ms=ms)
        md = g["mu_delta"].cpu().numpy()
        return bool(md[b, 0] >= 1e10 or not np.isfinite(float(g["grad"][b])))
    except Exception as e:   # (the check is a courtesy: a failure of it leaves the case flagged)
        print("pd_flip: %s" % e, flush=True)
        return False


def one(seed, nkinds=None, shapes="default"):
    cfg, prob, x0_q, x0_xi, us0 = draw(seed, nkinds, shapes)
    if isinstance(prob, tuple):
        prob, op = prob
    else:
        op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
    return (cfg,) + check(cfg, prob, op, x0_q, x0_xi, us0)


def check(cfg, prob, op, x0_q, x0_xi, us0, solver=None):
    """One case against the oracle: the GPU solve of cfg (mode, line_search, rollout, K = iterations, all of the batch) on
    prob, the oracle's on op, every trajectory compared with the classes below.  solver: a handle on prob to solve on
    (default: a fresh one of the case's batch).  Returns (worst_j, worst_u, notes, stats): the worst J / u distance in
    units of TOL_J / TOL_U times those, the disagreements no class accepts, and the count of each oracle status / class."""
    K, B = cfg["K"], cfg["B"]
    solver = BatchedTrackingILQR(prob, B) if solver is None else solver
    r = solver.fit_batch(x0_q, x0_xi, us0, mode=cfg["mode"], n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0,
                         line_search=cfg["line_search"], rollout=cfg["rollout"])
    kw = dict(mode=cfg["mode"], max_iter=K, line_search=cfg["line_search"], rollout=cfg["rollout"])
    o = ob.fit_batch(op, x0_q, x0_xi, us0, **kw)
    it, st, Jg, us = r.iters.cpu().numpy().copy(), r.status.cpu().numpy().copy(), r.J_hist.cpu().numpy(), r.us.cpu().numpy().copy()
    o["iters"], o["status"] = o["iters"].copy(), o["status"].copy()
    # the referee: the oracle's statements in long double.  nf[b, k] = how far the fp64 oracle has drifted from it by iteration k
    # (running maximum) -- the accuracy fp64 HAS on this trajectory; a trajectory on which the two take different decisions
    # (iteration counts, statuses) has no noise floor beyond that point: `forked`
    ref = obl.fit_batch(op, x0_q, x0_xi, us0, **kw) if REFEREE else None
    notes, worst_j, worst_u, stats = [], 0.0, 0.0, {}
    Ag = r.alpha_hist.cpu().numpy() if (r.alpha_hist is not None and (cfg["line_search"] or cfg["mode"] == "ss")) else None
    Mg = r.mu_hist.cpu().numpy() if getattr(r, "mu_hist", None) is not None else None
    Xg = r.xs_xi.cpu().numpy()
    searching = cfg["line_search"] or cfg["mode"] == "ss"
    tol_u0 = TOL_U if float(np.diag(prob.R)[: (4 if cfg["kind"] == "drone" else 3 if cfg["kind"] in ("so3", "pendulum") else 6)].min()) >= 1e-4 else TOL_U_FLAT
    for b in range(B):
        n = min(int(it[b]), int(o["iters"][b]))
        stats[int(o["status"][b])] = stats.get(int(o["status"][b]), 0) + 1
        jo = o["J_hist"][b, :max(n, 1)]
        finite = bool(np.isfinite(jo).all() and np.abs(jo).max() < 1e30)
        nf = np.zeros(max(n, 1))
        ref_agrees_gpu = ref_agrees_oracle = False
        if ref is not None:
            nr = min(n, int(ref["iters"][b]))
            with np.errstate(all="ignore"):
                d = np.abs((o["J_hist"][b, :nr].astype(obl.LD) - ref["J_hist"][b, :nr]) / ref["J_hist"][b, :nr]).astype(float)
            d = np.where(np.isfinite(d), d, np.inf)
            nf[:nr] = np.maximum.accumulate(d) if nr else 0.0
            nf[nr:] = np.inf   # the referee has stopped: the fp64 oracle is on its own from here
            ref_agrees_gpu = int(ref["iters"][b]) == int(it[b]) and int(ref["status"][b]) == int(st[b])
            ref_agrees_oracle = int(ref["iters"][b]) == int(o["iters"][b]) and int(ref["status"][b]) == int(o["status"][b])
        else:
            # without the referee: round 3's classification of what cannot be compared (overflowing costs, a cost that grows a
            # thousandfold in one accept-always iteration, gradients beyond 1e8)
            exploding = n > 1 and finite and (jo[1:] > 1e3 * np.abs(jo[:-1])).any()
            if exploding or not finite or (np.nanmax(np.abs(o["grad_hist"][b, :max(n, 1)])) > 1e8):
                nf[:] = np.inf
        if not finite:
            stats["nonfinite"] = stats.get("nonfinite", 0) + 1
        # ILL-CONDITIONED trajectories: a backward sweep whose regularisation ran away (mu >= 1e20 on either side: the sweep gave
        # up on a positive definite Q_uu at max_reg = 1e10 and the schedule of traopt_controller.py:2977-2995, carried from knot to
        # knot, kept multiplying -- every such case of the campaigns ended between 1e30 and 1e100), a cost that grows a
        # thousandfold in one accept-always iteration, or overflow.  Such a sweep solves INDEFINITE systems whose entries span
        # thirty and more orders of magnitude; the GPU's gains agree with the oracle's to ~1e-5 there (tools/_dbg_maxreg.py,
        # profiles/r04_parity_referee.txt) and what a line search then does with them differs.  Costs are compared up to the first
        # such iteration (with the referee's tolerance); exit codes and iteration counts are still compared and COUNTED
        # (`ill_exit_differs`), and fail the case only if one side reports a clean run (status 0) where the other reports a
        # failure.  (A max-regularisation exit that stays near 1e10 -- seed 30003 -- is NOT in this class: compared in full.)
        mu_o = o["mu_hist"][b, :max(n, 1)]
        mu_g = Mg[b, :max(n, 1)] if Mg is not None else mu_o
        bad_k = [k for k in range(n) if not np.isfinite(jo[k]) or abs(jo[k]) > 1e30 or mu_o[k] >= 1e20 or mu_g[k] >= 1e20
                 or o["grad_hist"][b, k] > 1e8   # (linearised a thousand rad/s away from anything: twists of 1e2 .. 1e12, seed 20144)
                 or (k > 0 and not searching and jo[k] > 1e3 * abs(jo[k - 1]))]
        # a rollout that has left the number range (twists beyond 1e6 rad/s on either side: seeds 20172, 20223 blow up in their
        # FIRST accept-always iteration, which no ratio of successive costs shows)
        diverged = float(np.abs(o["xs_xi"][b]).max()) > 1e6 or not np.isfinite(o["xs_xi"][b]).all() or float(np.nanmax(np.abs(Xg[b]))) > 1e6 \
            or not np.isfinite(Xg[b]).all()
        if diverged and not bad_k:
            bad_k = [0]
        if bad_k or not finite:
            stats["ill"] = stats.get("ill", 0) + 1
            n_cmp = min(bad_k) if bad_k else 0
            if it[b] != o["iters"][b] or st[b] != o["status"][b]:
                stats["ill_exit_differs"] = stats.get("ill_exit_differs", 0) + 1
                if (st[b] == 0) != (o["status"][b] == 0):
                    # ... unless the side that stayed clean takes the OTHER side's decision when it is given the other side's
                    # trajectory: the positive-definiteness test of one sweep hangs on the last digits of a trajectory the two
                    # agree on to 1e-15 (seeds 50312, 50349: profiles/r04c_parity_fuzz_final_tree.txt).  Counted, not hidden.
                    if pd_flip(b, solver, op, cfg, x0_q, x0_xi, us0, st, o, mu_g, mu_o, Jg):
                        stats["ill_pd_flip"] = stats.get("ill_pd_flip", 0) + 1
                    else:
                        notes.append("b%d (ill-conditioned) status %d/%d: one side clean, the other failed" % (b, st[b], o["status"][b]))
            if n_cmp:
                with np.errstate(all="ignore"):
                    e = np.abs(Jg[b, :n_cmp] - jo[:n_cmp]) / np.abs(jo[:n_cmp]) / np.maximum(TOL_J, 10.0 * nf[:n_cmp])
                worst_j = max(worst_j, float(np.nanmax(np.where(np.isfinite(e), e, 0.0))) * TOL_J)
            continue
        if n and cfg["mode"] == "ms" and cfg["line_search"]:
            # The merit function is J + w |d| with w re-derived every iteration from the expected change over |d|
            # (traopt_controller.py:2771-2788).  Once a trajectory is closed |d| is rounding noise (3e-16 here, 4e-15 in the
            # oracle, whose alpha = 1 rollout multiplies by factors that are the identity up to rounding: DESIGN section 3), w
            # is that noise's reciprocal, and which step size passes is decided by the noise: seed 7061, two SO(3) members
            # 1e-3 apart after agreeing to 1e-14 for seven iterations.  The comparison ends at the first such disagreement.
            a, c = Jg[b, :n], o["J_hist"][b, :n]
            with np.errstate(all="ignore"):
                off = np.nonzero(np.abs(a - c) > np.maximum(TOL_J, 10.0 * nf[:n]) * np.abs(c).max())[0]
            if off.size and o["defect_hist"][b, off[0]] < 1e-12:
                stats["merit_noise"] = stats.get("merit_noise", 0) + 1
                n = int(off[0])
                it[b] = o["iters"][b] = n   # (nothing behind it is comparable, the way the searches end included)
                st[b] = o["status"][b] = 0
                us[b] = o["us"][b]
                ref_agrees_gpu = ref_agrees_oracle = False
        if n:
            a, c = Jg[b, :n], o["J_hist"][b, :n]
            with np.errstate(all="ignore"):
                e = np.abs(a - c) / np.abs(c)
            e = np.where(np.isfinite(e), e, np.where(np.isfinite(a) == np.isfinite(c), 0.0, np.inf))   # same finiteness class
            if Ag is not None:
                # a search that ends up accepting steps of 1e-7 and below is deciding its Armijo test within a hundred
                # rounding errors of the cost: the two sides may then take DIFFERENT step sizes of that order (seed 2030:
                # costs 0.5 alpha apart behind two accepted steps of 7.7e-9) -- allow the sum of such steps so far
                tiny = np.cumsum(np.where(Ag[b, :n] < 1e-6, Ag[b, :n], 0.0))
                e = np.maximum(e - 10.0 * tiny, 0.0)
            # measured in units of the tolerance at that iteration: max(TOL_J, ten times the oracle's own distance from the referee)
            with np.errstate(all="ignore"):
                ee = e / np.maximum(TOL_J, 10.0 * nf[:n])
            ee = np.where(np.isnan(ee), 0.0, ee)
            if np.isinf(nf[:n]).any():
                stats["beyond_referee"] = stats.get("beyond_referee", 0) + 1
            worst_j = max(worst_j, float(ee.max()) * TOL_J)
        if it[b] != o["iters"][b] or st[b] != o["status"][b]:
            # the exit code and the iteration count are compared for EVERY trajectory, diverging ones included.  Accepted:
            # (1) the long-double referee takes the GPU's decision (the fp64 oracle's was the rounding one: seed 30003);
            # (2) the referee takes neither side's (three evaluations, three outcomes: decided by rounding);
            # (3) a search that has converged to rounding level ends on a coin flip (tests/test_gpu_matrix.py): the side that
            #     goes on does so without moving the cost
            longer = Jg[b, : it[b]] if it[b] > o["iters"][b] else o["J_hist"][b, : o["iters"][b]]
            tail = longer[max(n - 1, 0):]
            searching = cfg["line_search"] or cfg["mode"] == "ss"
            if ref is not None and ref_agrees_gpu:
                stats["oracle_rounding"] = stats.get("oracle_rounding", 0) + 1
            elif ref is not None and not ref_agrees_oracle:
                stats["three_way"] = stats.get("three_way", 0) + 1
            elif searching and len(tail) and np.isfinite(tail).all() and np.ptp(tail) <= 1e-10 * abs(tail[0]):   # (1e-11 in the hand-conditioned matrix test; 3.5e-11 seen in 47 000 random trajectories)
                stats["coin"] = stats.get("coin", 0) + 1
            else:
                notes.append("b%d iters %d/%d status %d/%d tail ptp %.1e" % (b, it[b], o["iters"][b], st[b], o["status"][b],
                                                                             np.ptp(tail) / abs(tail[0]) if len(tail) else -1))
        elif st[b] == 0 and np.isfinite(o["us"][b]).all():
            slack = 10.0 * float(np.where(Ag[b, :n] < 1e-6, Ag[b, :n], 0.0).sum()) if Ag is not None else 0.0
            scale = max(1.0, np.abs(o["us"][b]).max())
            eu = np.abs(us[b] - o["us"][b]).max() / scale
            nfu = 0.0
            if ref is not None and ref_agrees_oracle:
                nfu = float(np.abs(o["us"][b].astype(obl.LD) - ref["us"][b]).max()) / scale
            elif ref is not None:
                nfu = np.inf
            worst_u = max(worst_u, max(eu - slack, 0.0) / max(tol_u0, 10.0 * nfu) * TOL_U)
    return worst_j, worst_u, notes, stats


def main():
    global LARGE, REFEREE, NKINDS
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    LARGE = "--large" in flags
    shapes = "edge" if "--edge" in flags else "default"
    REFEREE = "--no-referee" not in flags
    for f in flags:
        if f.startswith("--kinds="):
            NKINDS = int(f.split("=")[1])
    n = int(args[0]) if len(args) > 0 else 100
    s0 = int(args[1]) if len(args) > 1 else 1000
    bad = 0
    status_total = {}
    for seed in range(s0, s0 + n):
        cfg, wj, wu, notes, stats = one(seed, shapes=shapes)
        for k, v in stats.items():
            status_total[k] = status_total.get(k, 0) + v
        flag = wj > TOL_J or wu > TOL_U or notes
        if flag:
            bad += 1
        print("%s seed %d %s  J %.1e  u %.1e  %s %s" % ("DIFF" if flag else "ok  ", seed, cfg, wj, wu, "; ".join(notes[:6]),
                                                          ("(+%d more)" % (len(notes) - 6)) if len(notes) > 6 else ""), flush=True)
    print("%d of %d cases differ (J and u in units of their tolerance x 1e-9 / 1e-6); over all trajectories: oracle statuses / classes: %s"
          % (bad, n, status_total))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
