"""What a pose schedule costs: the same solve timed with the batch-shared weights, with those weights given to every
trajectory as its own (tolg_set_weights, same numbers: the PT_W kernels with no schedule attached), and with a schedule on
top of them (tolg_set_pose_schedule: workloads.se3_gates' factors, 1 everywhere and gate_gain at the gate knots).

usage: python tools/bench_schedule.py [--lines headline,merit,ss] [--variants shared,weights,schedule] [--B 4096] [--N 200]
                                      [--gates 3] [--rounds 7] [--steps K] [--warmup W] [--out FILE.txt] [--dry]

One process, one handle per line; the variants are timed in alternation, round after round (the order rotates every round),
each region being iterations W .. W+K of a fresh solve between two device synchronisations (tools/_benchlib.py).  Per variant
the line reports the median time per iteration in ms, the fastest and slowest round, the spread (max - min) / median of the
rates, and the median over the shared variant's.  shared and weights are tools/bench_weights.py's shared and broadcast
variants: its figures on another commit are comparable with these.  In the line-search lines trajectories stop when they find
no descent, and a schedule changes which ones do: `active` says how many were still being solved at the end of each
variant's last region.  --out writes the table as text (profiles/pose_schedule_bench.txt)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import workloads  # noqa: E402
from _benchlib import LINES, add_common_args, print_row, rate_rounds, require_gpu, solve_rate_region, summary  # noqa: E402

VARIANTS = ("shared", "weights", "schedule")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "lines", lines="headline")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="a subset: one variant per process under a profiler")
    add_common_args(ap, "B", "N")
    ap.add_argument("--gates", type=int, default=3)
    add_common_args(ap, "rounds", "steps", "warmup", "out", "dry")
    a = ap.parse_args(argv)
    a.lines = a.lines.split(",")
    a.variants = tuple(v for v in VARIANTS if v in a.variants.split(","))
    bad = [x for x in a.lines if x not in LINES] or ([] if a.variants else ["no variant"])
    if bad or a.B < 1 or a.rounds < 1 or a.warmup < 0 or a.steps < 0 or not 1 <= a.gates < a.N:
        ap.error("lines from %s; variants from %s; rounds >= 1, warmup >= 0, steps >= 0, 1 <= gates < N" % (sorted(LINES), VARIANTS))
    return a


def inputs(a):
    """bench.py's batch (se3_tracking) and, per variant, its weights (or None) and schedule (or None): the problem's own
    weights once per trajectory, and se3_gates' factors for this batch."""
    prob, q0, xi0, us = workloads.se3_tracking(a.B, N=a.N)
    bc = tuple(np.broadcast_to(np.asarray(x, float), (a.B,) + np.shape(x)).copy() for x in (prob.Q, prob.P, prob.R))
    scale = workloads.se3_gates(a.B, N=a.N, gates=a.gates)[4]
    return prob, q0, xi0, us, {"shared": (None, None), "weights": (bc, None), "schedule": (bc, scale)}


def run_line(name, a, prob, q0, xi0, us, variants):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    dv = lambda x: None if x is None else torch.as_tensor(x, dtype=torch.float64, device=solver.device)  # noqa: E731
    q_d, xi_d, us_d = dv(q0), dv(xi0), dv(us)
    dev_in = {v: (None if w is None else tuple(dv(x) for x in w), s) for v, (w, s) in variants.items()}
    active, status_ok = {}, {}

    def region(v):
        w, s = dev_in[v]
        Q, P, R = w if w is not None else (None, None, None)
        # (the schedule is checked on the host by every call, outside the timed region)
        rate, res = solve_rate_region(solver, (q_d, xi_d, us_d), dict(Q=Q, P=P, R=R, pose_scale=s, **kw), W, K)
        active[v] = float((res.iters == W + K).double().mean().item())
        status_ok[v] = float((res.status == 0).double().mean().item())
        return rate

    rates = rate_rounds(a.variants, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, gates=a.gates, steps=K, warmup=W, rounds=a.rounds, unit="batch-iterations/s",
               variants={v: dict(summary(rates[v]), active=active[v], status_ok=status_ok[v]) for v in a.variants})
    base = out["variants"]["shared"]["median"] if "shared" in a.variants else float("nan")
    out["time_over_shared"] = {v: base / out["variants"][v]["median"] for v in a.variants}
    dev = solver.device
    del solver
    torch.cuda.synchronize(dev)
    return out


def table(results, variants):
    rows = ["%-9s %-9s %10s %10s %10s %8s %8s %7s %7s" % ("line", "variant", "ms/iter", "fastest", "slowest", "spread", "x shared",
                                                          "active", "ok")]
    for r in results:
        for v in variants:
            s = r["variants"][v]
            rows.append("%-9s %-9s %10.4f %10.4f %10.4f %7.2f%% %8.4f %7.3f %7.3f" % (
                r["line"], v, 1e3 / s["median"], 1e3 / s["max"], 1e3 / s["min"], 100 * s["spread"], r["time_over_shared"][v],
                s["active"], s["status_ok"]))
    return "\n".join(rows)


def main(argv=None):
    a = parse_args(argv)
    prob, q0, xi0, us, variants = inputs(a)
    if a.dry:
        s = variants["schedule"][1]
        print(json.dumps(dict(plan=a.lines, variants=a.variants, B=a.B, N=prob.N, gates=a.gates, rounds=a.rounds,
                              steps={n: a.steps or LINES[n][1] for n in a.lines}, warmup=a.warmup,
                              schedule_shape=list(s.shape), scaled_knots=int((s[:, :, 0] != 1.0).sum()))))
        return 0
    require_gpu("bench_schedule")
    results = []
    for name in a.lines:
        r = run_line(name, a, prob, q0, xi0, us, variants)
        results.append(r)
        print_row(r)
    head = ("tools/bench_schedule.py, one session on one MI355X (gfx950): B = %d, N = %d, %d gates, %d rounds in rotating order, "
            "median time per iteration (batch of B) of iterations W .. W+K of a fresh solve"
            % (a.B, a.N, a.gates, a.rounds))
    text = head + "\n\n" + table(results, a.variants) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
