"""Per-phase cycle stamps of the rollout (debug build: hipcc ... -DTOLG_STAMPS, loaded through TOLG_HIP_LIB)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, workloads  # noqa: E402
import stamp_rows  # noqa: E402

B, N, K = 4096, 200, 12
prob, x0_q, x0_xi, us0 = workloads.se3_tracking(B, N=N)
s = BatchedTrackingILQR(prob, B)
sched = sys.argv[1] if len(sys.argv) > 1 else "auto"   # auto: fused rollout + linearisation; split: rollout alone
r = s.fit_batch(x0_q, x0_xi, us0, mode="ms", n_iterations=K, tol_grad_norm=0.0, tol_d_norm=0.0, schedule=sched)
torch.cuda.synchronize()
st = stamp_rows.row(r.alpha_hist, stamp_rows.ROLL, 8)
if sched == "auto":  # roll_step_twist in wave 0 of k_rollout_lin
    names = ["loop overhead", "issue gains / controls reads (LDS)", "compose + Log(x^-1 x_new)", "K dx + quad broadcast",
             "twist half of the dynamics", "pose hand-over from the pose wave", "(unused)",
             "look-ahead (back-pressure, inputs, next nominal state) + publish + pose read"]
else:               # roll_step in k_rollout
    names = ["loop overhead + next-state prefetch issue", "issue gains / controls / factors loads", "Log(x^-1 x_new) + pose half",
             "K dx + quad broadcast", "twist half of the dynamics", "compose + project", "stores", "(unused)"]
tot = st[:8].sum()
print("schedule:", sched)
for n, v in zip(names, st):
    print("%-45s %8.0f cycles/knot  %5.1f %%" % (n, v / N, 100 * v / tot))
print("total per knot %.0f (s_memtime ticks)" % (tot / N))
if sched == "auto":
    pw = stamp_rows.row(r.alpha_hist, stamp_rows.POSE, 3) / N
    print("pose wave per knot: %.0f waiting for the twist, %.0f input DMA issue + publish, %.0f pose chain + publish" % tuple(pw))
    # helper h takes every second group of four knots (k_rollout_lin: ngroups, RL_NH = 2).  The passes are counted here, not
    # on the device: a helper that gave up early (TOLG_ST_INTERNAL) returns ahead of the flush, its row stays NaN; the
    # status is checked so that the averages are never taken over passes that did not run
    if int((r.status == 4).sum().item()):  # TOLG_ST_INTERNAL
        raise SystemExit("a wavefront of the fused launch gave up waiting (TOLG_ST_INTERNAL): no per-pass figures")
    for h in range(2):
        w, k = stamp_rows.row(r.alpha_hist, stamp_rows.HELPER + h, 2)
        n = len(range(h, (N + 1 + 3) // 4, 2))
        print("helper %d: %d passes, %.0f cycles per pass working, %.0f waiting for the rollout" % (h, n, k / max(n, 1), w / max(n, 1)))
