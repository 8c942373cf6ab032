"""What per-trajectory cost weights cost: the same solve timed with the batch-shared weights, with those weights given to
every trajectory as its own (tolg_set_weights, same numbers, the PT_W kernels), with K distinct weight sets
(workloads.se3_weight_sweep's sets, set b // (B / K)), and with those K sets together with R distinct references
(workloads.se3_multiref, reference b // (B / R): the PT_REF | PT_W kernels).

usage: python tools/bench_weights.py [--lines headline,merit,ss] [--variants shared,broadcast,distinct,refs]
                                     [--B 4096] [--N 200] [--sets 64] [--refs 64] [--rounds 7] [--steps K] [--warmup W]
                                     [--out FILE.json] [--dry]

One process, one handle per line; the variants are timed in alternation, round after round (the order rotates every
round), each region being iterations W .. W+K of a fresh solve between two device synchronisations.  Per variant the
line reports the median rate (batch iterations per second), the lowest and highest, and the spread (max - min) / median;
per line the median rate of each variant over the shared one's.  Lines: headline = SE3 multiple shooting, accept-always,
schedule auto (bench.py's metric configuration); merit = the merit line search; ss = single shooting.  In the line-search
lines trajectories stop when they find no descent, and distinct weights change which ones do: the broadcast variant is
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

VARIANTS = ("shared", "broadcast", "distinct", "refs")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "lines")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="a subset: one variant per process under a profiler")
    add_common_args(ap, "B", "N")
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--refs", type=int, default=64)
    add_common_args(ap, "rounds", "steps", "warmup", "out", "dry")
    a = ap.parse_args(argv)
    a.lines = a.lines.split(",")
    a.variants = tuple(v for v in VARIANTS if v in a.variants.split(","))
    bad = [x for x in a.lines if x not in LINES] or ([] if a.variants else ["no variant"])
    if (bad or a.B < 1 or a.refs < 1 or a.sets < 1 or a.B % a.refs or a.B % a.sets or a.rounds < 1 or a.warmup < 0
            or a.steps < 0):
        ap.error("lines from %s; B a multiple of refs and of sets; rounds >= 1, warmup >= 0, steps >= 0" % sorted(LINES))
    return a


def inputs(a):
    """Per variant: initial states, references (or None) and weights (or None).  shared / broadcast / distinct: bench.py's
    batch (se3_tracking); refs: the same batch moved with its references (workloads.se3_multiref)."""
    prob, q0, xi0, us, _, _, _, _, (Qk, Pk, Rk) = workloads.se3_weight_sweep(a.B, a.sets, N=a.N)
    ws = np.arange(a.B) // (a.B // a.sets)
    distinct = (Qk[ws], Pk[ws], Rk[ws])
    bc = tuple(np.broadcast_to(np.asarray(x, float), (a.B,) + np.shape(x)).copy() for x in (prob.Q, prob.P, prob.R))
    ri = np.arange(a.B) // (a.B // a.refs)
    _, q, xi, _, q_ref, xi_ref, _, _ = workloads.se3_multiref(a.B, a.refs, N=a.N, index=ri)
    return prob, us, {"shared": (q0, xi0, None, None, None), "broadcast": (q0, xi0, None, None, bc),
                      "distinct": (q0, xi0, None, None, distinct), "refs": (q, xi, q_ref, xi_ref, distinct)}


def run_line(name, a, prob, us, variants):
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR
    kw, K0 = LINES[name]
    K, W = a.steps or K0, a.warmup
    solver = BatchedTrackingILQR(prob, a.B)
    f64 = dict(dtype=torch.float64, device=solver.device)
    us_d = torch.as_tensor(us, **f64)
    dv = lambda x: None if x is None else torch.as_tensor(x, **f64)  # noqa: E731
    dev_in = {v: (dv(t[0]), dv(t[1]), dv(t[2]), dv(t[3]), None if t[4] is None else tuple(dv(x) for x in t[4]))
              for v, t in variants.items()}
    V = a.variants
    active, status_ok = {}, {}

    def region(v):
        q_d, xi_d, qr, xr, w = dev_in[v]
        Q, P, R = w if w is not None else (None, None, None)
        rate, res = solve_rate_region(solver, (q_d, xi_d, us_d), dict(q_ref=qr, xi_ref=xr, Q=Q, P=P, R=R, **kw), W, K)
        active[v] = float((res.iters == W + K).double().mean().item())
        status_ok[v] = float((res.status == 0).double().mean().item())
        return rate

    rates = rate_rounds(V, region, a.rounds)
    out = dict(line=name, B=a.B, N=a.N, sets=a.sets, refs=a.refs, steps=K, warmup=W, rounds=a.rounds, unit="batch-iterations/s",
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
        print(json.dumps(dict(plan=a.lines, B=a.B, N=prob.N, sets=a.sets, refs=a.refs, rounds=a.rounds,
                              steps={n: a.steps or LINES[n][1] for n in a.lines}, warmup=a.warmup,
                              distinct_sets=int(len(np.unique(variants["distinct"][4][0][:, 0, 0]))),
                              distinct_references=int(len(np.unique(variants["refs"][2][:, 0, 0, 3]))))))
        return 0
    require_gpu("bench_weights")
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
