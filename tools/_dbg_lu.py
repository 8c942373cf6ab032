"""max-regularisation LU branch, unit level: gains of one backward sweep, GPU vs fp64 oracle vs long-double oracle (the set-up of
tests/test_gpu_parity.py::test_regularisation_loop_nonpd_branch: an indefinite R makes Q_uu non-PD)."""
import sys, numpy as np
sys.path.insert(0, '.')
np.set_printoptions(precision=2, linewidth=220)
from oracle import bridge as ob, bridge_ld as obl
from trajectory_optimization_matrix_lie_groups_amd import BatchedTrackingILQR, TrackingProblem, workloads
prob, *_ = workloads.se3_tracking(1, N=16)
R = np.diag([-30.0, 1e-3, 1e-3, -5.0, 1e-3, 1e-3])
prob = TrackingProblem("se3", prob.J, prob.dt, prob.Q, R, prob.P, prob.q_ref, prob.xi_ref)
B = 4
rng = np.random.default_rng(5)
from tests.support import random_traj
xs_q, xs_xi, us = random_traj(prob, B, seed=5, spread=0.1)
op = ob.OracleProblem(prob.kind, prob.J, prob.dt, prob.Q, prob.R, prob.P, prob.q_ref, prob.xi_ref)
r = BatchedTrackingILQR(prob, B).linearize_backward(xs_q, xs_xi, us, ms=True)
for b in range(B):
    o = ob.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=True)
    l = obl.lin_backward(op, xs_q[b], xs_xi[b], us[b], ms=True)
    Kg, Ko, Kl = r["K"][b].cpu().numpy(), o["K"], l["K"].astype(float)
    sc = np.abs(Kl).max(axis=(1, 2))
    print("b%d mu %.3e/%.3e/%.3e  rel K error per knot (N-1 .. 0):" % (b, float(r["mu_delta"][b, 0]), o["mu"], float(l["mu"])))
    print("   GPU-ld   ", (np.abs(Kg - Kl).max(axis=(1, 2)) / sc)[::-1])
    print("   oracle-ld", (np.abs(Ko - Kl).max(axis=(1, 2)) / sc)[::-1])
