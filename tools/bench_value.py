"""What the cost-to-go of the held policy costs (tolg_policy_value) beside its forward twin (tolg_policy_covariance) and beside
one sampled closed loop (tolg_policy_rollout, S = 1): a solved 4096 x 200 SE3 tracking batch.

usage: python tools/bench_value.py [--B 4096] [--N 200] [--rounds 7] [--iters 10] [--out FILE.json]

One process.  The batch is solved once, untimed (multiple shooting, accept-always, 20 iterations).  Then, round after round,
the cases are timed in alternation: `iters` back-to-back calls between two events, through the C ABI (no host-side input
checks).  Cases: the value with its reduced outputs (p, diag_P, price, excess), the value with price and excess only (p is
skipped), the covariance with its reduced outputs (var_x, var_u, pos_cov), and tolg_policy_rollout at S = 1 (J and status
only).  Reported per case: the median ms per call over the rounds, min and max, and the ratio to tolg_policy_rollout at S = 1."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import workloads  # noqa: E402
from _benchlib import add_common_args, emit, event_rounds, print_row, stats_row  # noqa: E402

CASES = {"value": "tolg_policy_value (p, diag_P, price, excess)", "value_excess": "tolg_policy_value (price, excess)",
         "covariance": "tolg_policy_covariance (var_x, var_u, pos_cov)", "rollout": "tolg_policy_rollout S=1"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "B", "N", "rounds", "iters", "out", iters=10)
    a = ap.parse_args(argv)
    if a.B < 1 or a.N < 1 or a.rounds < 1 or a.iters < 1:
        ap.error("B, N, rounds, iters >= 1")
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR

    B, N = a.B, a.N
    prob, q, xi, us, S0, W = workloads.se3_covariance(B, N=N)
    m = prob.m
    s = BatchedTrackingILQR(prob, B)
    s.fit_batch(q, xi, us, mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
    torch.cuda.synchronize()
    dev = s.device
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    f64 = dict(dtype=torch.float64, device=dev)
    d_S0, d_W = torch.as_tensor(S0, **f64), torch.as_tensor(W, **f64)
    pv, diag_P = torch.empty(B, N + 1, 12, **f64), torch.empty(B, N + 1, 12, **f64)
    price, excess = torch.empty(B, N, **f64), torch.empty(B, **f64)
    var_x, var_u, pos = torch.empty(B, N + 1, 12, **f64), torch.empty(B, N, m, **f64), torch.empty(B, N + 1, 6, **f64)
    dx0 = torch.randn(B, 1, 12, generator=g, **f64) * 0.05
    w = torch.randn(B, 1, N, 6, generator=g, **f64) * 0.01
    J, st = torch.empty(B, 1, **f64), torch.empty(B, 1, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(name):
        if name == "value":
            return s.lib.tolg_policy_value(s._h, B, p(d_S0), p(d_W), None, p(pv), p(diag_P), p(price), p(excess), s._stream())
        if name == "value_excess":
            return s.lib.tolg_policy_value(s._h, B, p(d_S0), p(d_W), None, None, None, p(price), p(excess), s._stream())
        if name == "covariance":
            return s.lib.tolg_policy_covariance(s._h, B, p(d_S0), p(d_W), None, p(var_x), p(var_u), p(pos), s._stream())
        return s.lib.tolg_policy_rollout(s._h, B, 1, p(dx0), p(w), p(J), p(st), None, None, None, s._stream())

    names = list(CASES)
    times = event_rounds(names, call, a.rounds, a.iters)
    base = stats_row(times["rollout"])["ms_median"]
    rows = []
    for n in names:
        row = dict(case=CASES[n], **stats_row(times[n]))
        row["ratio_to_rollout_S1"] = row["ms_median"] / base
        rows.append(row)
        print_row(row)
    finite = bool(all(torch.isfinite(t).all().item() for t in (pv, diag_P, price, excess)))
    res = dict(B=B, N=N, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(dev), outputs_finite=finite, rows=rows)
    print_row(dict(outputs_finite=finite))
    emit(res, a.out)
    return res


if __name__ == "__main__":
    main()
