"""What per-trajectory references cost: the same solve timed with the batch-shared reference, with that reference given
to every trajectory as its own (tolg_set_refs, same numbers, the PTREF kernels), and with R distinct references
(workloads.se3_multiref, reference b // (B / R)).

usage: python tools/bench_multiref.py [--lines headline,merit,ss] [--variants shared,broadcast,distinct] [--B 4096]
                                      [--N 200] [--refs 64] [--rounds 7] [--steps K] [--warmup W] [--out FILE.json] [--dry]

One process, one handle per line; the three variants are timed in alternation, round after round (the order rotates every
round), each region being iterations W .. W+K of a fresh solve between two device synchronisations.  Per variant the
line reports the median rate (batch iterations per second), the lowest and highest, and the spread (max - min) / median;
per line the median rate of each variant over the shared one's.  Lines: headline = SE3 multiple shooting, accept-always,
schedule auto (bench.py's metric configuration); merit = the merit line search; ss = single shooting.  In the line-search
lines trajectories stop when they find no descent, and distinct references change which ones do: the broadcast variant is
the like-for-like one there, `active` says how many were still being solved at the end of each variant's last region,
`status_ok` how many ended it with TOLG_ST_OK."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import workloads  # noqa: E402
from _benchlib import LINES, add_common_args, emit, print_row, rate_rounds, require_gpu, solve_rate_region, summary  # noqa: E402

VARIANTS = ("shared", "broadcast", "distinct")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "lines")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="a subset: one variant per process under a profiler")
    add_common_args(ap, "B", "N")
    ap.add_argument("--refs", type=int, default=64)
    add_common_args(ap, "rounds", "steps", "warmup", "out", "dry")
    a = ap.parse_args(argv)
    a.lines = a.lines.split(",")
    a.variants = tuple(v for v in VARIANTS if v in a.variants.split(","))
    bad = [x for x in a.lines if x not in LINES] or ([] if a.variants else ["no variant"])
    if bad or a.B < 1 or a.refs < 1 or a.B % a.refs or a.rounds < 1 or a.warmup < 0 or a.steps < 0:
        ap.error("lines from %s; B a multiple of refs; rounds >= 1, warmup >= 0, steps >= 0" % sorted(LINES))
    return a


def inputs(a):
    """Per variant: initial states and references.  shared / broadcast: bench.py's batch (se3_tracking); distinct: the same
    batch moved with its references (workloads.se3_multiref), each trajectory placed relative to its own reference."""
    idx = np.arange(a.B) // (a.B // a.refs)
    prob, q, xi, us, q_ref, xi_ref, idx, G = workloads.se3_multiref(a.B, a.refs, N=a.N, index=idx)
    _, q0, xi0, _ = workloads.se3_tracking(a.B, N=a.N)
    q_bc = np.broadcast_to(prob.q_ref, q_ref.shape).copy()
    xi_bc = np.broadcast_to(prob.xi_ref, xi_ref.shape).copy()
    return prob, us, {"shared": (q0, xi0, None, None), "broadcast": (q0, xi0, q_bc, xi_bc), "distinct": (q, xi, q_ref, xi_ref)}


def run_line(name, a, prob, us, variants):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    f64 = dict(dtype=torch.float64, device=solver.device)
    us_d = torch.as_tensor(us, **f64)
    dev_in = {v: tuple(None if x is None else torch.as_tensor(x, **f64) for x in t) for v, t in variants.items()}
    V = a.variants
    active, status_ok = {}, {}

    def region(v):
        q_d, xi_d, qr, xr = dev_in[v]
        rate, res = solve_rate_region(solver, (q_d, xi_d, us_d), dict(q_ref=qr, xi_ref=xr, **kw), W, K)
        active[v] = float((res.iters == W + K).double().mean().item())
        status_ok[v] = float((res.status == 0).double().mean().item())
        return rate

    rates = rate_rounds(V, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, refs=a.refs, steps=K, warmup=W, rounds=a.rounds, unit="batch-iterations/s",
               variants={v: dict(summary(rates[v]), active=active[v], status_ok=status_ok[v]) for v in V})
    base = out["variants"]["shared"]["median"] if "shared" in V else float("nan")
    out["ratio_to_shared"] = {v: out["variants"][v]["median"] / base for v in V}
    dev = solver.device
    del solver
    torch.cuda.synchronize(dev)
    return out


def main(argv=None):
    a = parse_args(argv)
    prob, us, variants = inputs(a)
    if a.dry:
        print(json.dumps(dict(plan=a.lines, B=a.B, N=prob.N, refs=a.refs, rounds=a.rounds,
                              steps={n: a.steps or LINES[n][1] for n in a.lines}, warmup=a.warmup,
                              distinct_references=int(len(np.unique(variants["distinct"][2][:, 0, 0, 3]))))))
        return 0
    require_gpu("bench_multiref")
    results = []
    for name in a.lines:
        r = run_line(name, a, prob, us, variants)
        results.append(r)
        print_row(r)
    print("%-9s %-10s %10s %10s %10s %8s %7s %7s %7s" % ("line", "variant", "median", "min", "max", "spread", "ratio", "active",
                                                       "ok"))
    for r in results:
        for v in a.variants:
            s = r["variants"][v]
            print("%-9s %-10s %10.1f %10.1f %10.1f %7.2f%% %7.4f %7.3f %7.3f" % (
                r["line"], v, s["median"], s["min"], s["max"], 100 * s["spread"], r["ratio_to_shared"][v], s["active"],
                s["status_ok"]))
    emit(results, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
