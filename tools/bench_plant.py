"""What a plant costs the closed loops (tolg_set_plant): tolg_policy_rollout of a solved 4096 x 200 SE3 tracking batch with
no plant, a diagonal plant per sample, a dense (rotated) plant per sample and a diagonal plant per trajectory (S_plant = 1),
and one tolg_mpc_advance step with and without a diagonal plant.

usage: python tools/bench_plant.py [--B 4096] [--N 200] [--S 1,16,64] [--rounds 7] [--iters 20] [--out FILE.json]

One process, one handle.  The batch is solved once, untimed (multiple shooting, accept-always, 20 iterations).  Then, round
after round, every (variant, S) pair is timed in alternation by tools/_benchlib.py's event_rounds: the pair's plant is attached
(tolg_set_plant, outside the timed region), then `iters` back-to-back calls between two events, through the C ABI.  Reported
per pair: the median ms per call over the rounds, min and max, and the bytes of plant rows the call reads."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import _capi, workloads  # noqa: E402
from _benchlib import add_common_args, emit, event_rounds, print_row, stats_row  # noqa: E402

VARIANTS = ("none", "diag", "dense", "diag_traj")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_common_args(ap, "B", "N", "S", "rounds", "iters", "out")
    a = ap.parse_args(argv)
    a.S = [int(s) for s in a.S.split(",")]
    if a.B < 1 or a.N < 1 or min(a.S) < 1 or a.rounds < 1 or a.iters < 1:
        ap.error("B, N, S, rounds, iters >= 1")
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR

    B, N = a.B, a.N
    prob, q, xi, us = workloads.se3_tracking(B, N=N)
    s = BatchedTrackingILQR(prob, B)
    s.fit_batch(q, xi, us, mode="ms", n_iterations=20, tol_grad_norm=0.0, tol_d_norm=0.0)
    torch.cuda.synchronize()
    dev = s.device
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    f64 = dict(dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    inputs, plants = {}, {}
    for S in a.S:
        dx0 = torch.randn(B, S, 12, generator=g, **f64) * 0.05
        w = torch.randn(B, S, N, 6, generator=g, **f64) * 0.01
        inputs[S] = (dx0, w, torch.empty(B, S, **f64), torch.empty(B, S, dtype=torch.int32, device=dev))
        for v, rot, Sp in (("diag", False, S), ("dense", True, S), ("diag_traj", False, 1)):
            PJ = workloads.plant_mismatch(B, Sp, N=N, sigma_inertia=0.1, rotate=rot, seed=11)[6]
            J, _, form, _ = s._check_plant(B, PJ, None, per_sample=True)
            assert form == (_capi.PLANT_DENSE if rot else _capi.PLANT_DIAG)
            buf = torch.empty(int(s.lib.tolg_plant_bytes(C.byref(s._p), B, Sp)) // 8, **f64)
            plants[(v, S)] = (torch.as_tensor(J, **f64), form, Sp, buf)
    mpc_plant = plants[("diag_traj", a.S[0])]
    warm = tuple(torch.empty(*shape, **f64) for shape in ((B, N + 1, 4, 4), (B, N + 1, 6), (B, N, prob.m)))
    x_next = tuple(torch.empty(*shape, **f64) for shape in ((B, 4, 4), (B, 6), (B, prob.m)))

    def attach(n):
        v = n[0]
        if v in ("none", "mpc_none"):
            return s.lib.tolg_set_plant(s._h, 0, 0, 0, None, None, None, 0, s._stream())
        J, form, Sp, buf = mpc_plant if v == "mpc_diag" else plants[n]
        return s.lib.tolg_set_plant(s._h, B, Sp, form, p(J), None, p(buf), C.c_size_t(buf.numel() * 8), s._stream())

    def call(n):
        if n[0].startswith("mpc"):
            return s.lib.tolg_mpc_advance(s._h, B, None, *map(p, x_next), *map(p, warm), None, s._stream())
        dx0, w, J, st = inputs[n[1]]
        return s.lib.tolg_policy_rollout(s._h, B, n[1], p(dx0), p(w), p(J), p(st), None, None, None, s._stream())

    names = [(v, S) for S in a.S for v in VARIANTS] + [("mpc_none", 1), ("mpc_diag", 1)]
    times = event_rounds(names, call, a.rounds, a.iters, attach=attach)
    attach(("none", 1))
    rows = []
    base = {S: statistics.median(times[("none", S)]) for S in a.S}
    for n in names:
        v, S = n
        row = dict(kernel="tolg_mpc_advance" if v.startswith("mpc") else "tolg_policy_rollout", variant=v, S=S,
                   **stats_row(times[n]))
        med = row["ms_median"]
        if not v.startswith("mpc"):
            Sp = 0 if v == "none" else plants[n][2]
            fields = 0 if v == "none" else (38 if v == "dense" else 14)
            row.update(vs_none=med / base[S], plant_bytes=B * Sp * fields * 8,
                       steps_per_s=B * S * N / (med * 1e-3))
        rows.append(row)
        print_row(row)
    res = dict(B=B, N=N, rounds=a.rounds, iters=a.iters, device=torch.cuda.get_device_name(dev), rows=rows)
    emit(res, a.out)
    return res


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
