"""What keep-out spheres cost: the same solve timed without spheres and with K = 1, 4, 8 spheres per trajectory
(workloads.se3_obstacle_field, tolg_set_al_obstacles: the PT_OBS kernels), plus one augmented-Lagrangian solve
(al_fit_batch(obstacles=...)) on the K = 8 field: its outer-iteration count and time.

usage: python tools/bench_obstacles.py [--lines headline,merit,ss] [--Ks 0,1,4,8] [--B 4096] [--N 200] [--rounds 7]
                                       [--steps K] [--warmup W] [--al] [--moving] [--kinds] [--pose] [--box] [--out FILE.json]
                                       [--dry]

One process, one handle per line; the variants are timed in alternation, round after round (the order rotates every round),
each region being iterations W .. W+K of a fresh solve between two device synchronisations (tools/_benchlib.py's
solve_rate_region and rate_rounds, as in tools/bench_weights.py).  The multipliers are fixed (lambda 0.1, I_mu 1e-2: what
the first outer iteration of al_fit_batch sees, with lambda > 0 so that no term is zero).  Per variant the line reports the
median rate (batch iterations per second), the lowest and highest, the spread (max - min) / median, and the median over the
no-sphere variant's.

--moving sends the same field of each K, repeated over the N + 1 knots, through tolg_set_al_obstacles_moving ([B, N+1, K, 4]):
the same arithmetic on geometry that is streamed per knot instead of read from 4K cached values, so the lines beside the
static ones show what the streaming costs.

--kinds times what the per-slot kind costs (tolg_set_al_obstacle_kinds) at K = 6 slots in place of the K sweep: no slots, all
keep-out spheres (workloads.se3_obstacle_field with K = 6: the K = 6 run of this tool without the flag), the corridor mix
(workloads.se3_corridor: two half-spaces, a geofence, two columns, a sphere) and all half-spaces (the tangent planes of the
spheres that face the start of the path).  One line per mix for every solve line asked for.

--pose times what the second slot family costs (tolg_set_al_pose_constraints) in place of the K sweep: nothing attached, the
two pose slots of workloads.se3_inspection (a tilt cone and a view cone whose target drifts: the per-knot form), six keep-out
spheres, and both families together.

--box times what the forms of the input box cost (tolg_set_al, tolg_set_al_box) in place of the K sweep, the same bounds in
every variant (+-10, workloads.al_tracking's, under lambda 0.1, I_mu 1e-2): no box; the shared [m] box, which runs the kernels
without PT_OBS; the same box as [B, m] and as [B, N, m], which select the PT_OBS forms with no slot attached; and, beside six
keep-out spheres (the PT_OBS forms in every variant), the shared box (read with strides 0), [B, m] and [B, N, m]."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import workloads  # noqa: E402
from _benchlib import LINES, add_common_args, emit, print_row, rate_rounds, require_gpu, solve_rate_region, summary  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "lines")
    ap.add_argument("--Ks", default="0,1,4,8", help="spheres per trajectory of each variant (0: none attached)")
    add_common_args(ap, "B", "N", "rounds", "steps", "warmup")
    ap.add_argument("--al", action="store_true", help="also time one al_fit_batch on the K = max(Ks) field")
    ap.add_argument("--moving", action="store_true", help="attach each field per knot (tolg_set_al_obstacles_moving)")
    ap.add_argument("--kinds", action="store_true", help="time the kind mixes at K = 6 (spheres, corridor, half-spaces)")
    ap.add_argument("--pose", action="store_true", help="time two pose slots (tilt cone, view cone) alone and beside six spheres")
    ap.add_argument("--box", action="store_true", help="time the forms of the input box, alone and beside six spheres")
    add_common_args(ap, "out", "dry")
    a = ap.parse_args(argv)
    a.lines = a.lines.split(",")
    a.Ks = tuple(int(k) for k in a.Ks.split(","))
    if any(x not in LINES for x in a.lines) or any(not 0 <= k <= 16 for k in a.Ks) or a.B < 1 or a.rounds < 1:
        ap.error("lines from %s; 0 <= K <= 16; B, rounds >= 1" % sorted(LINES))
    return a


def run_line(name, a, prob, q0, xi0, us, obs):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    dev = solver.device
    f64 = dict(dtype=torch.float64, device=dev)
    q_d, xi_d, us_d = (torch.as_tensor(x, **f64) for x in (q0, xi0, us))
    mult = {k: (torch.full((a.B, a.N + 1, k), 0.1, **f64), torch.full((a.B, a.N + 1, k), 1e-2, **f64)) for k in a.Ks if k}

    field = {}
    if a.moving:  # the field of each K at every knot, on the device once
        field = {k: torch.as_tensor(obs[:, None, :k], **f64).expand(a.B, a.N + 1, k, 4).contiguous() for k in a.Ks if k}

    def region(k):
        if k:
            solver.set_al_obstacles(field[k] if a.moving else obs[:, :k], *mult[k])
        rate, _ = solve_rate_region(solver, (q_d, xi_d, us_d), kw, W, K)
        if k:
            solver.set_al_obstacles(None)
            torch.cuda.synchronize(dev)
        return rate

    rates = rate_rounds(a.Ks, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, steps=K, warmup=W, rounds=a.rounds, moving=a.moving, unit="batch-iterations/s",
               variants={"K=%d" % k: summary(rates[k]) for k in a.Ks})
    if 0 in a.Ks:
        base = out["variants"]["K=0"]["median"]
        out["ratio_to_none"] = {v: s["median"] / base for v, s in out["variants"].items()}
    del solver
    torch.cuda.synchronize(dev)
    return out


KIND_MIXES = ("none", "spheres", "corridor", "half_spaces")


def kind_mixes(a):
    """{mix: (obstacles [B, 6, 4], kinds)} on se3_tracking's workload, which se3_obstacle_field and se3_corridor share"""
    import numpy as np
    prob, q0, xi0, us, sph = workloads.se3_obstacle_field(a.B, 6, N=a.N)
    cor, kinds = workloads.se3_corridor(a.B, N=a.N)[4:]
    n = sph[..., :3] - prob.q_ref[0, :3, 3]
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    planes = np.concatenate([n, np.sum(n * sph[..., :3], axis=-1, keepdims=True) - sph[..., 3:]], axis=-1)
    return (prob, q0, xi0, us), {"spheres": (sph, None), "corridor": (cor, kinds), "half_spaces": (planes, ("half_space",) * 6)}


def run_kinds_line(name, a, prob, q0, xi0, us, mixes):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    dev = solver.device
    f64 = dict(dtype=torch.float64, device=dev)
    q_d, xi_d, us_d = (torch.as_tensor(x, **f64) for x in (q0, xi0, us))
    mult = (torch.full((a.B, a.N + 1, 6), 0.1, **f64), torch.full((a.B, a.N + 1, 6), 1e-2, **f64))

    def region(mix):
        if mix != "none":
            solver.set_al_obstacles(mixes[mix][0], *mult, kinds=mixes[mix][1])
        rate, _ = solve_rate_region(solver, (q_d, xi_d, us_d), kw, W, K)
        if mix != "none":
            solver.set_al_obstacles(None)
            torch.cuda.synchronize(dev)
        return rate

    rates = rate_rounds(KIND_MIXES, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, K=6, steps=K, warmup=W, rounds=a.rounds, unit="batch-iterations/s",
               variants={m: summary(rates[m]) for m in KIND_MIXES})
    base = out["variants"]["none"]["median"]
    out["ratio_to_none"] = {v: s["median"] / base for v, s in out["variants"].items()}
    del solver
    torch.cuda.synchronize(dev)
    return out


POSE_MIXES = ("none", "pose", "spheres", "both")


def run_pose_line(name, a, prob, q0, xi0, us, sph, slots, kinds):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    dev = solver.device
    f64 = dict(dtype=torch.float64, device=dev)
    q_d, xi_d, us_d = (torch.as_tensor(x, **f64) for x in (q0, xi0, us))
    mult = {k: (torch.full((a.B, a.N + 1, k), 0.1, **f64), torch.full((a.B, a.N + 1, k), 1e-2, **f64)) for k in (2, 6)}
    slots_d = torch.as_tensor(slots, **f64)

    def region(mix):
        if mix in ("spheres", "both"):
            solver.set_al_obstacles(sph, *mult[6])
        if mix in ("pose", "both"):
            solver.set_al_pose_constraints(slots_d, kinds, *mult[2])
        rate, _ = solve_rate_region(solver, (q_d, xi_d, us_d), kw, W, K)
        solver.set_al_pose_constraints(None)
        solver.set_al_obstacles(None)
        torch.cuda.synchronize(dev)
        return rate

    rates = rate_rounds(POSE_MIXES, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, K=6, pose_K=2, steps=K, warmup=W, rounds=a.rounds, unit="batch-iterations/s",
               variants={m: summary(rates[m]) for m in POSE_MIXES})
    base = out["variants"]["none"]["median"]
    out["ratio_to_none"] = {v: s["median"] / base for v, s in out["variants"].items()}
    del solver
    torch.cuda.synchronize(dev)
    return out


BOX_MIXES = ("none", "shared", "trajectory", "knot", "spheres", "spheres+shared", "spheres+trajectory", "spheres+knot")


def run_box_line(name, a, prob, q0, xi0, us, sph):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    dev = solver.device
    f64 = dict(dtype=torch.float64, device=dev)
    q_d, xi_d, us_d = (torch.as_tensor(x, **f64) for x in (q0, xi0, us))
    m = prob.m
    mult = (torch.full((a.B, a.N + 1, 6), 0.1, **f64), torch.full((a.B, a.N + 1, 6), 1e-2, **f64))
    bmult = (torch.full((a.B, a.N, 2 * m), 0.1, **f64), torch.full((a.B, a.N, 2 * m), 1e-2, **f64))
    shape = {"shared": (m,), "trajectory": (a.B, m), "knot": (a.B, a.N, m)}
    box = {k: (torch.full(v, -10.0, **f64), torch.full(v, 10.0, **f64)) for k, v in shape.items()}

    def region(mix):
        form = mix.split("+")[-1]
        if mix.startswith("spheres"):
            solver.set_al_obstacles(sph, *mult)
        if form in box:
            solver.set_al(*box[form], *bmult)
        rate, _ = solve_rate_region(solver, (q_d, xi_d, us_d), kw, W, K)
        solver.set_al(None)
        solver.set_al_obstacles(None)
        torch.cuda.synchronize(dev)
        return rate

    rates = rate_rounds(BOX_MIXES, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, K=6, steps=K, warmup=W, rounds=a.rounds, unit="batch-iterations/s",
               variants={v: summary(rates[v]) for v in BOX_MIXES})
    base = out["variants"]["none"]["median"]
    out["ratio_to_none"] = {v: s["median"] / base for v, s in out["variants"].items()}
    del solver
    torch.cuda.synchronize(dev)
    return out


def run_al(a, prob, q0, xi0, us, obs):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    solver = BatchedTrackingILQR(prob, a.B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res, info = solver.al_fit_batch(q0, xi0, us, n_al_iters=20, n_ilqr_iters=200, obstacles=obs, tol_constr=1e-2)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    return dict(line="al_fit_batch", B=a.B, N=a.N, K=obs.shape[1], seconds=t, outer_iterations=info["outer_iterations"],
                al_converged=float(info["al_converged"].double().mean().item()),
                max_violation_max=float(info["max_violation"].max().item()),
                inner_converged=float((res.converged != 0).double().mean().item()))


def main(argv=None):
    a = parse_args(argv)
    kmax = max(max(a.Ks), 1)
    prob, q0, xi0, us, obs = workloads.se3_obstacle_field(a.B, kmax, N=a.N)
    if a.kinds:
        (prob, q0, xi0, us), mixes = kind_mixes(a)
    if a.pose:  # (se3_tracking's starts and path under both workloads: the slots fit the sphere field's problem)
        prob, q0, xi0, us, sph6 = workloads.se3_obstacle_field(a.B, 6, N=a.N)
        slots, pose_kinds = workloads.se3_inspection(a.B, N=a.N)[4:]
    if a.box:
        prob, q0, xi0, us, sph6 = workloads.se3_obstacle_field(a.B, 6, N=a.N)
    if a.dry:
        print(json.dumps(dict(plan=a.lines, Ks=a.Ks, B=a.B, N=prob.N, rounds=a.rounds, al=a.al, moving=a.moving,
                              kinds=list(KIND_MIXES) if a.kinds else None, pose=list(POSE_MIXES) if a.pose else None,
                              box=list(BOX_MIXES) if a.box else None,
                              steps={n: a.steps or LINES[n][1] for n in a.lines}, warmup=a.warmup)))
        return 0
    require_gpu("bench_obstacles")
    results = []
    for name in a.lines:
        if a.box:
            r = run_box_line(name, a, prob, q0, xi0, us, sph6)
        elif a.pose:
            r = run_pose_line(name, a, prob, q0, xi0, us, sph6, slots, pose_kinds)
        else:
            r = run_kinds_line(name, a, prob, q0, xi0, us, mixes) if a.kinds else run_line(name, a, prob, q0, xi0, us, obs)
        results.append(r)
        print_row(r)
    if a.al:
        r = run_al(a, prob, q0, xi0, us, obs)
        results.append(r)
        print_row(r)
    print("%-9s %-18s %10s %10s %10s %8s %7s" % ("line", "K", "median", "min", "max", "spread", "ratio"))
    for r in results:
        for v, s in r.get("variants", {}).items():
            print("%-9s %-18s %10.1f %10.1f %10.1f %7.2f%% %7.4f" % (r["line"], v, s["median"], s["min"], s["max"],
                                                                   100 * s["spread"], r.get("ratio_to_none", {}).get(v, float("nan"))))
    emit(results, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
