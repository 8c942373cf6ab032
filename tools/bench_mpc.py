"""What a receding-horizon MPC step costs (BatchedTrackingILQR.mpc), and how many iterations a step needs with warm states
against warm controls.

usage: python tools/bench_mpc.py [--B 4096] [--N 200,50] [--iters 0,1,3,5] [--steps 20] [--rounds 5]
                                 [--tol-steps 10] [--tol-rounds 2] [--max-iters 30] [--out FILE.json]
       python tools/bench_mpc.py --constrained [--B 4096] [--N 200] [--K 4] [--iters 5] [--steps 20] [--rounds 5]
                                 [--loops unconstrained,box,spheres,box+spheres,pose,spheres+pose]
       python tools/bench_mpc.py --estimated [--B 4096] [--N 200] [--mask 0x03F] [--steps 20] [--rounds 5]

One process, se3_mpc's workload (every trajectory its own path and phase, twist disturbances behind every step), multiple
shooting, accept-always.

- Step times: for every N and every `iters` k, `steps` closed-loop steps with k iterations each (the first step too,
  first_iters = k), warm="states", check_every = 0 -- no host read inside the loop --, timed from a device synchronisation
  before the call to one after it.  The (N, k) pairs alternate round after round; reported: the median ms per step over the
  rounds, min, max, and MPC steps per second (B trajectory-steps per step).  k = 0 is the pure overhead of a step: windows,
  begin (the initial guess and the first linearisation), end and advance.
- Iterations per step: `tol-steps` steps under tolerances (tol_grad_norm = tol_d_norm = 1e-6, check_every = 1, at most
  `max-iters` iterations a step, the first step 50), warm="states" and warm="controls" on the same paths and disturbances,
  alternated `tol-rounds` times.  Reported: mean iterations per step over steps 1.. (step 0 is cold for both), its maximum,
  the fraction of (trajectory, step) solves that stopped below the cap, and ms per step.
- --constrained: se3_mpc_obstacles' workload instead.  For every N and k the unconstrained loop and the loops with the planner's
  box (the 90th percentile of the unconstrained loop's inputs), with K spheres per trajectory on world-time paths (a device
  tensor, as the reference paths), with both, with the two pose slots of se3_mpc_inspection on world-time paths (the same paths,
  starts and disturbances: both workloads are se3_mpc's) and with spheres and pose slots (first_al_iters = al_iters_per_step =
  1: the same iteration count) alternate round after round in one process; reported as above, with each loop's solves of status
  OK, its last step's largest violation, its least clearance and its least pose margin.  Then the step kernel alone:
  tolg_al_mpc_step (shift = 1) on the last plan with the box and sphere multiplier sets attached, and again with the pose slots as
  the third set (tolg_al_mpc_step_pose), `steps` calls between two device synchronisations.  The pose loops cap mu at 1 (mu_max): the path leaves the
  cones for good, mu would grow at every step, and accept-always iterations diverge under a penalty that large; what a step
  costs does not depend on mu.  --loops runs a subset of the loops (an A/B against a build without the pose loops runs the same
  four in both).
- --estimated: what output feedback adds to a step.  On se3_mpc_estimated's workload and a held policy, with an actuator box
  on: the pair tolg_mpc_measure + tolg_mpc_advance_estimated, and tolg_mpc_advance_limited alone, `steps` calls each between two
  device synchronisations on preallocated buffers (the loop's own path: no host work per call), alternated round after round
  behind a warm-up round; then, on the same handle, one accept-always solver iteration (tolg_solve_iterate(steps) inside a
  solve in flight, per iteration).  Reported: the median ms per call (pair: per pair) over the rounds, min, max, and the two
  ratios pair / limited and pair / iteration."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import workloads  # noqa: E402
from _benchlib import add_common_args, emit, print_row, rotated, stats_row  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "B")
    ap.add_argument("--N", default="200,50")
    ap.add_argument("--iters", default="0,1,3,5")
    ap.add_argument("--steps", type=int, default=20)
    add_common_args(ap, "rounds", rounds=5)
    ap.add_argument("--tol-steps", type=int, default=10)
    ap.add_argument("--tol-rounds", type=int, default=2)
    ap.add_argument("--max-iters", type=int, default=30)
    ap.add_argument("--constrained", action="store_true")
    ap.add_argument("--estimated", action="store_true")
    ap.add_argument("--mask", type=lambda x: int(x, 0), default=0x03F)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--loops", default="unconstrained,box,spheres,box+spheres,pose,spheres+pose")
    add_common_args(ap, "out")
    a = ap.parse_args(argv)
    a.N = [int(x) for x in a.N.split(",")]
    a.iters = [int(x) for x in a.iters.split(",")]
    if a.B < 1 or min(a.N) < 1 or min(a.iters) < 0 or a.steps < 1 or a.rounds < 1 or a.tol_steps < 2 or a.tol_rounds < 1:
        ap.error("B, N, steps, rounds >= 1; iters >= 0; tol-steps >= 2")
    return a


def constrained(a):
    """The constrained loop beside the unconstrained one (--constrained)"""
    import numpy as np
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR

    B, zero, rows = a.B, dict(tol_grad_norm=0.0, tol_d_norm=0.0), []
    for N in a.N:
        prob, q, xi, pq, px, t0, noise, obs, mov = workloads.se3_mpc_obstacles(B, a.steps, N=N, K=a.K)
        s = BatchedTrackingILQR(prob, B)
        dev = lambda x: torch.as_tensor(x, device=s.device)  # noqa: E731
        inp = dict(x0_q=q, x0_xi=xi, path_q=dev(pq), path_xi=dev(px), t0=t0, noise=noise, steps=a.steps, warm="states",
                   check_every=0, **zero)
        mov_d = dev(mov)
        pose_paths, pose_kinds = workloads.se3_mpc_inspection(B, a.steps, N=N)[7:]
        pose_d = dev(pose_paths)
        for k in a.iters:
            free = s.mpc(first_iters=k, iters_per_step=k, **inp)
            u = np.abs(free.us.cpu().numpy())
            lim = np.percentile(u[np.isfinite(u).all(axis=(1, 2))].reshape(-1, prob.m), 90, axis=0)
            al = dict(first_al_iters=1, al_iters_per_step=1)
            loops = {"unconstrained": {}, "box": dict(lb=-lim, ub=lim, **al), "spheres": dict(obstacle_paths=mov_d, **al),
                     "box+spheres": dict(lb=-lim, ub=lim, obstacle_paths=mov_d, **al),
                     "pose": dict(pose_paths=pose_d, pose_kinds=pose_kinds, mu_max=1.0, **al),
                     "spheres+pose": dict(obstacle_paths=mov_d, pose_paths=pose_d, pose_kinds=pose_kinds, mu_max=1.0, **al)}
            loops = {name: loops[name] for name in a.loops.split(",")}
            times = {name: [] for name in loops}
            last = {}
            for r in range(a.rounds + 1):  # round 0 warms up
                for name in rotated(list(times), r):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    last[name] = s.mpc(first_iters=k, iters_per_step=k, **loops[name], **inp)
                    torch.cuda.synchronize()
                    if r:
                        times[name].append((time.perf_counter() - t) * 1e3 / a.steps)
            for name, res in last.items():
                st = stats_row(times[name], "ms_per_step")
                row = dict(part="constrained_step_time", loop=name, N=N, K=a.K, iters_per_step=k, **st,
                           status_ok=int((res.status == 0).sum().item()), solves=B * a.steps)
                if res.max_violation is not None:
                    row.update(max_violation_last_step=float(res.max_violation[:, -1].max().item()), mu_max=float(res.mu.max().item()))
                if res.clearance is not None:
                    row.update(min_clearance=float(res.clearance.min().item()))
                if res.pose_margin is not None:
                    row.update(min_pose_margin=float(res.pose_margin.min().item()))
                rows.append(row)
                print_row(row)
        # the step kernel alone, on a plan and both multiplier sets
        f64 = dict(dtype=torch.float64, device=s.device)
        plan = s.fit_batch(q, xi, None, n_iterations=3, check_every=0, **zero)
        lam, imu = torch.zeros(B, N, 2 * prob.m, **f64), torch.full((B, N, 2 * prob.m), 1e-2, **f64)
        s.set_al(-lim, lim, lam, imu)
        s.set_al_obstacle_windows(mov_d, 0, t0=t0, lam=None, imu=torch.full((B, N + 1, a.K), 1e-2, **f64))
        mu = torch.full((B,), 1e-2, **f64)
        moved = 8 * B * (2 * 2 * (N * 2 * prob.m + (N + 1) * a.K) + 2 * N * prob.m + 2 * (3 + 4 * a.K) * (N + 1))
        Kp = pose_paths.shape[2]
        for part in ("al_mpc_step_alone", "al_mpc_step_alone_with_pose")[:2 if "pose" in a.loops else 1]:
            if part.endswith("pose"):  # the third row set: its multipliers twice; per pass the rest of the pose and its geometry
                s.set_al_pose_constraint_windows(pose_d, 0, t0=t0, kinds=pose_kinds, imu=torch.full((B, N + 1, Kp), 1e-2, **f64))
                moved += 8 * B * (2 * 2 * (N + 1) * Kp + 2 * (9 + 4 * Kp) * (N + 1))
            ms = []
            for r in range(a.rounds + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.steps):
                    s.al_mpc_step(plan.xs_q, plan.us, mu, shift=True)
                torch.cuda.synchronize()
                if r:
                    ms.append((time.perf_counter() - t) * 1e3 / a.steps)
            row = dict(part=part, N=N, K=a.K, **stats_row(ms, "ms_per_call"), bytes_needed=moved)
            rows.append(row)
            print_row(row)
        s.set_al(None)
        s.set_al_obstacles(None)
        s.set_al_pose_constraints(None)
    res = dict(B=B, N=a.N, K=a.K, steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(0), rows=rows)
    emit(res, a.out)
    return res


def estimated(a):
    """measure + advance_estimated against advance_limited and one solver iteration (--estimated)"""
    import numpy as np
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR

    B, zero, rows = a.B, dict(tol_grad_norm=0.0, tol_d_norm=0.0), []
    for N in a.N:
        prob, q, xi, pq, px, t0, noise, est = workloads.se3_mpc_estimated(B, a.steps, N=N)
        s = BatchedTrackingILQR(prob, B)
        dev = lambda x: s._dev(x, np.shape(x))  # noqa: E731
        r = s.fit_batch(q, xi, None, n_iterations=3, check_every=0, **zero)
        u0 = np.abs(r.us[:, 0].cpu().numpy())
        lim = np.percentile(u0[np.isfinite(u0).all(axis=1)], 90, axis=0)
        box = (dev(np.broadcast_to(-lim, (B, prob.m)).copy()), dev(np.broadcast_to(lim, (B, prob.m)).copy()))
        V, W, n, w = dev(est["meas_V"]), dev(est["est_W"]), dev(est["meas_noise"][:, 0]), dev(noise[:, 0])
        xt_q, xt_xi = r.xs_q[:, 0].reshape(B, 16).clone(), r.xs_xi[:, 0].clone()
        e_q, e_xi, P = xt_q.clone(), xt_xi.clone(), dev(est["est_Sigma0"])
        innov, var = torch.empty(B, 12, dtype=torch.float64, device=s.device), torch.empty(B, 12, dtype=torch.float64, device=s.device)
        adv = s._advance_out(B, torch.zeros(B, dtype=torch.float64, device=s.device), limited=True)

        def pair():
            s._measure(B, a.mask, V, xt_q, xt_xi, n, e_q, e_xi, P, None, innov, var)
            s._advance_est(B, w, box, xt_q, xt_xi, P, W, adv)

        parts = {"measure+advance_estimated": pair, "advance_limited": lambda: s._advance(B, w, adv, box)}
        times = {name: [] for name in parts}
        for rnd in range(a.rounds + 1):  # round 0 warms up
            for name in rotated(list(parts), rnd):
                xt_q.copy_(r.xs_q[:, 0].reshape(B, 16)); xt_xi.copy_(r.xs_xi[:, 0]); P.copy_(dev(est["est_Sigma0"]))
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.steps):
                    parts[name]()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t) * 1e3 / a.steps)
        s.solve_begin(q, xi, None, mode="ms", n_iterations=a.steps * (a.rounds + 1), histories=False, **zero)
        times["solver_iteration"] = []
        for rnd in range(a.rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            s.solve_iterate(a.steps)
            torch.cuda.synchronize()
            if rnd:
                times["solver_iteration"].append((time.perf_counter() - t) * 1e3 / a.steps)
        s.solve_end()
        med = {}
        for name, ms in times.items():
            st = stats_row(ms, "ms_per_call")
            med[name] = st["ms_per_call_median"]
            row = dict(part="estimated", what=name, N=N, mask="%#05x" % a.mask, **st)
            rows.append(row)
            print_row(row)
        row = dict(part="estimated_ratios", N=N, pair_over_advance_limited=med["measure+advance_estimated"] / med["advance_limited"],
                   pair_over_solver_iteration=med["measure+advance_estimated"] / med["solver_iteration"])
        rows.append(row)
        print_row(row)
    res = dict(B=B, N=a.N, steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(0), rows=rows)
    emit(res, a.out)
    return res


def main(argv=None):
    a = parse_args(argv)
    if a.constrained:
        return constrained(a)
    if a.estimated:
        return estimated(a)
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR

    B = a.B
    zero = dict(tol_grad_norm=0.0, tol_d_norm=0.0)
    cases = {}
    for N in a.N:
        steps = max(a.steps, a.tol_steps)
        prob, q, xi, pq, px, t0, noise = workloads.se3_mpc(B, steps, N=N)
        s = BatchedTrackingILQR(prob, B)
        inp = dict(x0_q=q, x0_xi=xi, path_q=torch.as_tensor(pq, device=s.device), path_xi=torch.as_tensor(px, device=s.device),
                   t0=t0)
        cases[N] = (s, inp, noise)

    def timed(N, k):
        s, inp, noise = cases[N]
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = s.mpc(steps=a.steps, first_iters=k, iters_per_step=k, warm="states", noise=noise[:, :a.steps], check_every=0,
                  **inp, **zero)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / a.steps, r

    pairs = [(N, k) for N in a.N for k in a.iters]
    for n, k in pairs:  # warm-up: code objects, allocator, the refs buffer
        timed(n, k)
    times = {p: [] for p in pairs}
    status_ok = {}
    for r in range(a.rounds):
        for p in rotated(pairs, r):
            ms, res = timed(*p)
            times[p].append(ms)
            status_ok[p] = int((res.status == 0).sum().item())
    rows = []
    for p in pairs:
        st = stats_row(times[p], "ms_per_step")
        med = st["ms_per_step_median"]
        row = dict(part="step_time", N=p[0], iters_per_step=p[1], **st, mpc_steps_per_s=1e3 / med,
                   trajectory_steps_per_s=B * 1e3 / med, status_ok=status_ok[p], solves=B * a.steps)
        rows.append(row)
        print_row(row)

    tol = dict(tol_grad_norm=1e-6, tol_d_norm=1e-6)
    for N in a.N:
        s, inp, noise = cases[N]
        acc = {w: [] for w in ("controls", "states")}
        for r in range(a.tol_rounds):
            for warm in (("controls", "states") if r % 2 == 0 else ("states", "controls")):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = s.mpc(steps=a.tol_steps, first_iters=50, iters_per_step=a.max_iters, warm=warm,
                            noise=noise[:, :a.tol_steps], check_every=1, **inp, **tol)
                torch.cuda.synchronize()
                acc[warm].append(((time.perf_counter() - t) * 1e3 / a.tol_steps, res.iters.cpu().numpy(),
                                  int((res.status == 0).sum().item())))
        for warm in ("controls", "states"):
            it = acc[warm][-1][1][:, 1:]
            row = dict(part="iterations", N=N, warm=warm, steps=a.tol_steps, iters_cap=a.max_iters,
                       mean_iters_per_step=float(it.mean()), max_iters_per_step=int(it.max()),
                       mean_iters_step0=float(acc[warm][-1][1][:, 0].mean()),
                       below_cap=float((it < a.max_iters).mean()),
                       ms_per_step_median=statistics.median(x[0] for x in acc[warm]),
                       same_iters_every_round=all((x[1] == acc[warm][0][1]).all() for x in acc[warm]),
                       status_ok=acc[warm][-1][2], solves=B * a.tol_steps)
            rows.append(row)
            print_row(row)
    res = dict(B=B, N=a.N, steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(0), rows=rows)
    emit(res, a.out)
    return res


if __name__ == "__main__":
    main()
