"""What the feature benches (tools/bench_<feature>.py) share: the solve-rate lines and their timed region, the event-timed
rounds, the alternation order, the statistics of a row, the repeated command-line flags and the --out file.  torch is
imported inside the functions that time, so the argument parsing and --dry paths need no GPU."""
import json
import os
import statistics
import time

# line -> (fit keywords, timed iterations per region)
LINES = {
    "headline": (dict(mode="ms", line_search=False, schedule="auto"), 300),
    "merit": (dict(mode="ms", line_search=True, schedule="auto"), 100),
    "ss": (dict(mode="ss", line_search=False, schedule="auto"), 60),
}

_FLAGS = {
    "lines": dict(default="headline,merit,ss"),
    "B": dict(type=int, default=4096),
    "N": dict(type=int, default=200),
    "S": dict(default="1,16,64"),
    "rounds": dict(type=int, default=7),
    "iters": dict(type=int, default=20, help="calls per timed region"),
    "steps": dict(type=int, default=0, help="timed iterations per region (0: the line's default)"),
    "warmup": dict(type=int, default=5),
    "out": dict(default=None),
    "dry": dict(action="store_true", help="build the inputs and print the plan; no GPU"),
}


def add_common_args(ap, *names, **defaults):
    """Add --<name> for each name, in the order given (the order of --help); defaults: another default for a flag."""
    for n in names:
        kw = dict(_FLAGS[n])
        if n in defaults:
            kw["default"] = defaults[n]
        ap.add_argument("--" + n, **kw)


def summary(rates):
    med = statistics.median(rates)
    return dict(median=med, min=min(rates), max=max(rates), spread=(max(rates) - min(rates)) / med, runs=rates)


def stats_row(times, prefix="ms"):
    """{prefix_median, prefix_min, prefix_max} of one case's per-round times."""
    return {prefix + "_median": statistics.median(times), prefix + "_min": min(times), prefix + "_max": max(times)}


def rotated(seq, r):
    """seq started at element r (mod its length): the order of round r, so that every case leads equally often."""
    return seq[r % len(seq):] + seq[:r % len(seq)]


def require_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s: no GPU visible (there is nothing to time on the CPU)" % tool)


def solve_rate_region(solver, begin_args, begin_kwargs, W, K):
    """Iterations W .. W+K of a fresh solve with zero tolerances between two device synchronisations.
    Returns (batch iterations per second, the FitResult of solve_end); the device is idle on return."""
    import torch
    dev = solver.device
    solver.solve_begin(*begin_args, n_iterations=W + K, tol_grad_norm=0.0, tol_d_norm=0.0, **begin_kwargs)
    solver.solve_iterate(W)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    solver.solve_iterate(K)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    res = solver.solve_end()
    torch.cuda.synchronize(dev)
    return K / (t1 - t0), res


def rate_rounds(variants, region, rounds):
    """region(v) -> rate.  One untimed pass over the variants (every kernel of every variant loaded and run once), then
    `rounds` passes in rotating order.  Returns {variant: [rate per round]}."""
    for v in variants:
        region(v)
    rates = {v: [] for v in variants}
    for r in range(rounds):
        for v in rotated(variants, r):
            rates[v].append(region(v))
    return rates


def event_rounds(names, call, rounds, iters, attach=None):
    """call(name) -> 0 launches one case through the C ABI.  Every case once as warm-up and argument check, then `rounds`
    passes in rotating order, each case timed as `iters` back-to-back calls between two events.  attach(name), if given,
    runs before the case, outside the timed region, with a synchronise behind it.  Returns {name: [ms per call per round]}."""
    import torch
    for n in names:
        if (attach is not None and attach(n) != 0) or call(n) != 0:
            raise RuntimeError("launch failed: %s" % (n,))
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds):
        for n in rotated(names, r):
            if attach is not None:
                attach(n)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                call(n)
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) / iters)
    return times


def print_row(row):
    print(json.dumps(row), flush=True)


def emit(results, out):
    """Write the results to the --out file, if one was asked for (its directory is created)."""
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
