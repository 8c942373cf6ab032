"""Host side of the batched solver: PyTorch-ROCm tensors in, C ABI (include/tolg.h) underneath.

PyTorch is plumbing here (device memory, streams, torch.distributed); every flop of the hot path
runs in the hand-written HIP kernels of csrc/tolg_kernels.hip.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _capi

_KIND = {"se3": _capi.DYN_SE3, "rigidbody": _capi.DYN_RIGIDBODY, "drone": _capi.DYN_DRONE, "so3": _capi.DYN_SO3,
         "pendulum3d": _capi.DYN_PENDULUM3D}


@dataclass
class TrackingProblem:
    """One (dynamics, cost) pair shared by the batch.

    Mirrors the constructor arguments of SE3Dynamics / RigidBodyDynamics / DroneDynamics
    (reference traoptlibrary/traopt_dynamics.py:633, :906, :1214) and
    SE3TrackingQuadraticGaussNewtonCost (traoptlibrary/traopt_cost.py:587)."""
    kind: str
    J: np.ndarray
    dt: float
    Q: np.ndarray
    R: np.ndarray
    P: np.ndarray
    q_ref: np.ndarray   # (N+1, 4, 4)
    xi_ref: np.ndarray  # (N+1, 6)
    pend_mass: float = 0.0    # Pendulum3dDyanmics m, length (traopt_dynamics.py:425); other kinds ignore them
    pend_length: float = 0.0

    @property
    def N(self):
        return int(np.asarray(self.q_ref).shape[0]) - 1

    @property
    def m(self):
        return 4 if self.kind == "drone" else 6


def embed_so3(J3, dt, Q6, R3, P6, R_ref, w_ref) -> TrackingProblem:
    """SO(3) tracking problem in the SE(3) layout of the C ABI (include/tolg.h, TOLG_DYN_SO3):
    zero translation / linear velocity / inputs 3..5, J = blkdiag(J_so3, I3), R = blkdiag(R_so3, I3)."""
    R_ref = np.asarray(R_ref, float); w_ref = np.asarray(w_ref, float)
    n = R_ref.shape[0]
    J = np.eye(6); J[:3, :3] = J3
    Q = np.zeros((12, 12)); Q[:3, :3] = np.asarray(Q6)[:3, :3]; Q[6:9, 6:9] = np.asarray(Q6)[3:, 3:]
    P = np.zeros((12, 12)); P[:3, :3] = np.asarray(P6)[:3, :3]; P[6:9, 6:9] = np.asarray(P6)[3:, 3:]
    R = np.eye(6); R[:3, :3] = R3
    q_ref = np.tile(np.eye(4), (n, 1, 1)); q_ref[:, :3, :3] = R_ref
    xi_ref = np.zeros((n, 6)); xi_ref[:, :3] = w_ref
    return TrackingProblem("so3", J, float(dt), Q, R, P, q_ref, xi_ref)


def embed_pendulum3d(J3, mass, length, dt, Q6, R3, P6, R_ref, w_ref) -> TrackingProblem:
    """Pendulum3dDyanmics (reference traoptlibrary/traopt_dynamics.py:421-626) with the SO3 tracking cost, in
    the same embedding as embed_so3 (include/tolg.h, TOLG_DYN_PENDULUM3D); the pivot acceleration is u[0:3]."""
    p = embed_so3(J3, dt, Q6, R3, P6, R_ref, w_ref)
    p.kind, p.pend_mass, p.pend_length = "pendulum3d", float(mass), float(length)
    return p


@dataclass
class FitResult:
    xs_q: torch.Tensor      # [B, N+1, 4, 4]
    xs_xi: torch.Tensor     # [B, N+1, 6]
    us: torch.Tensor        # [B, N, m]
    J_hist: torch.Tensor    # [B, max_iter]
    grad_hist: torch.Tensor  # [B, max_iter+1]
    defect_hist: torch.Tensor  # [B, max_iter+1]
    alpha_hist: torch.Tensor
    mu_hist: torch.Tensor
    iters: torch.Tensor     # [B] int32
    status: torch.Tensor    # [B] int32
    converged: torch.Tensor  # [B] int32
    extra: dict = field(default_factory=dict)


@dataclass
class PolicyRollout:
    """S closed-loop rollouts per trajectory of the held policy (BatchedTrackingILQR.policy_rollout)."""
    J: torch.Tensor        # [B, S] tracking cost of each sample
    status: torch.Tensor   # [B, S] int32: ST_OK or ST_NONFINITE
    xs_q: Optional[torch.Tensor] = None   # [B, S, N+1, 4, 4] (trajectories=True)
    xs_xi: Optional[torch.Tensor] = None  # [B, S, N+1, 6]
    us: Optional[torch.Tensor] = None     # [B, S, N, m]
    # policy_rollout(u_lb=, u_ub=): the applied inputs that differ from the commanded ones, and the margin the box lacked
    n_sat: Optional[torch.Tensor] = None           # [B, S] int32
    u_excess: Optional[torch.Tensor] = None        # [B, S]
    # policy_rollout(clearance=True): min over knots and slots of the clearance of the slot's kind (a keep-out sphere: |t - c| - r;
    # kind_clearance), and the first knot that attains it
    clearance: Optional[torch.Tensor] = None       # [B, S]
    clearance_knot: Optional[torch.Tensor] = None  # [B, S] int32
    # pose_margin=True: min over knots and pose slots of the slot's margin (pose_margin(); negative: outside a cone), and the
    # first knot that attains it
    pose_margin: Optional[torch.Tensor] = None       # [B, S]
    pose_margin_knot: Optional[torch.Tensor] = None  # [B, S] int32
    # violations=True: per knot, the samples whose clearance (viol_pos) / pose margin (viol_pose) is below zero there; each
    # for the family attached (rollout_margins is the definition)
    viol_pos: Optional[torch.Tensor] = None          # [B, N+1] int32
    viol_pose: Optional[torch.Tensor] = None         # [B, N+1] int32
    # policy_rollout_estimated(estimates=True): the filter's posterior estimates x^_i (xs_q / xs_xi hold the true states)
    est_q: Optional[torch.Tensor] = None           # [B, S, N+1, 4, 4]
    est_xi: Optional[torch.Tensor] = None          # [B, S, N+1, 6]
    # policy_rollout(act_*=): the commands c_i behind which the applied inputs `us` lag (commands=True), the inputs the rate
    # limit moved, and the largest distance between a command and the input applied at its knot
    u_cmd: Optional[torch.Tensor] = None           # [B, S, N, m]
    n_rate: Optional[torch.Tensor] = None          # [B, S] int32
    u_gap: Optional[torch.Tensor] = None           # [B, S]


@dataclass
class PolicyCovarianceEstimated:
    """Covariance of the held policy under output feedback (BatchedTrackingILQR.policy_covariance_estimated): the loop acts on
    the estimate of a Kalman filter with coordinate measurements.  Coordinates and layout as PolicyCovariance."""
    var_x: torch.Tensor                     # [B, N+1, 12] diag Sigma_i, the true state's variance
    var_est: torch.Tensor                   # [B, N+1, 12] diag P^+_i, the estimation error's variance after the knot's update
    var_u: torch.Tensor                     # [B, N, m] diag K_i S^_i^+ K_i^T
    mask: int = 0                           # the measured coordinates, as the device took them
    pos_cov: Optional[torch.Tensor] = None  # [B, N+1, 3, 3] world-frame position covariance from Sigma: what inflate_obstacles takes
    Sigma: Optional[torch.Tensor] = None    # [B, N+1, 12, 12] (full=True)
    P_post: Optional[torch.Tensor] = None   # [B, N+1, 12, 12] (full=True)
    L: Optional[torch.Tensor] = None        # [B, N+1, 12, 12] the Kalman gains (gains=True): policy_rollout_estimated's input


@dataclass
class PolicyCovariance:
    """First-order closed-loop covariance of the held policy (BatchedTrackingILQR.policy_covariance), in the error coordinates
    of the gains; for so3 and the pendulum in the embedded 12-coordinate layout gains() uses (3..5 and 9..11 unused)."""
    var_x: torch.Tensor                     # [B, N+1, 12] diag Sigma_i
    var_u: torch.Tensor                     # [B, N, m] diag K_i Sigma_i K_i^T
    pos_cov: Optional[torch.Tensor] = None  # [B, N+1, 3, 3] world-frame position covariance (None for so3 and the pendulum)
    Sigma: Optional[torch.Tensor] = None    # [B, N+1, 12, 12] (full=True)


@dataclass
class PolicyValue:
    """Cost-to-go of the held policy (BatchedTrackingILQR.policy_value), V_i(e) ~ p_i . e + e^T P_i e / 2 in the error
    coordinates of the gains; for so3 and the pendulum in the embedded 12-coordinate layout gains() uses (3..5 and 9..11 unused)."""
    p: torch.Tensor                     # [B, N+1, 12]; p[:, 0] is the gradient of the closed-loop cost in the start error
    diag_P: torch.Tensor                # [B, N+1, 12] diag P_i
    price: torch.Tensor                 # [B, N] tr(P_{i+1}[6:12, 6:12] W) / 2: what the disturbance behind step i costs
    excess: torch.Tensor                # [B] tr(P_0 Sigma0) / 2 + sum_i price_i: expected closed-loop cost above the nominal's
    P: Optional[torch.Tensor] = None    # [B, N+1, 12, 12] (full=True)


def check_covariance(name, a, B, n, compact=None):
    """A covariance input of policy_covariance checked on the host: `a` is [B, n, n] or [n, n] (broadcast over the batch), or
    with compact = (k, index) also [B, k, k] / [k, k], embedded at rows / columns `index` of an n x n zero matrix.  It must be
    finite, symmetric (to 1e-12 of its largest entry) and positive semi-definite (eigvalsh >= -1e-12 * its largest
    eigenvalue); ValueError otherwise, before anything reaches the device.  Returns a float64 [B, n, n] numpy array."""
    a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    sizes = (n,) + ((compact[0],) if compact else ())
    if a.ndim not in (2, 3) or a.shape[-1] != a.shape[-2] or a.shape[-1] not in sizes or (a.ndim == 3 and a.shape[0] != B):
        raise ValueError("%s has shape %s, expected (%d, %s, %s) or (%s, %s) with n = %s"
                         % (name, tuple(a.shape), B, "n", "n", "n", "n", " or ".join(map(str, sizes))))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s must be finite" % name)
    a = np.broadcast_to(a, (B,) + a.shape[-2:])
    scale = np.abs(a).max(axis=(1, 2), keepdims=True)
    if np.any(np.abs(a - np.swapaxes(a, 1, 2)) > 1e-12 * scale):
        raise ValueError("%s must be symmetric" % name)
    ev = np.linalg.eigvalsh(0.5 * (a + np.swapaxes(a, 1, 2)))
    if np.any(ev[:, 0] < -1e-12 * np.maximum(ev[:, -1], 0.0)) or np.any(ev[:, -1] < 0.0):
        raise ValueError("%s must be positive semi-definite" % name)
    if a.shape[-1] != n:
        idx = np.asarray(compact[1])
        full = np.zeros((B, n, n))
        full[:, idx[:, None], idx[None, :]] = a
        a = full
    return np.ascontiguousarray(a)


_SO3_COORDS = [0, 1, 2, 6, 7, 8]  # where the SO3 family's (rotation, omega) sit in the 12-coordinate layout


def measurement_mask(mask, so3=False):
    """The measured coordinates as the 12-bit int the device takes: `mask` is such an int, or an iterable of coordinate indices
    0..11; ValueError for anything else, and for coordinates 3..5 / 9..11 of the SO3 family (so3: no translation)."""
    if isinstance(mask, (int, np.integer)) and not isinstance(mask, bool):
        m = int(mask)
        if m < 0 or m > 0xFFF:
            raise ValueError("mask has 12 bits, one per coordinate of the error state: %r" % (mask,))
    else:
        m = 0
        try:
            idx = [j for j in mask]
        except TypeError:
            raise ValueError("mask must be an int or an iterable of coordinate indices: %r" % (mask,)) from None
        for j in idx:
            if not isinstance(j, (int, np.integer)) or isinstance(j, bool) or j < 0 or j > 11:
                raise ValueError("mask holds coordinate indices 0..11: %r" % (j,))
            m |= 1 << int(j)
    if so3 and (m & 0xE38):
        raise ValueError("the SO3 family has no translation or linear velocity: coordinates 3..5 and 9..11 cannot be measured")
    return m


def check_measurement(mask, V, B, so3=False):
    """The measurement model of policy_covariance_estimated / policy_rollout_estimated checked on the host; ValueError before
    anything reaches the device.  mask: an int whose bit j says that coordinate j of the error state is measured (12 bits), or an
    iterable of coordinate indices 0..11.  V: the measurement-noise variances, [12] (every trajectory the same) or [B, 12]; on a
    measured coordinate finite and > 0, on an unmeasured one ignored (whatever it holds; it goes to the device as 0); None is
    allowed when nothing is measured.  so3: the problem is of the SO3 family -- the translation and linear-velocity coordinates
    3..5 and 9..11 cannot be measured, and V may also be [6] or [B, 6] over (rotation, omega), embedded at 0..2 and 6..8 as
    check_covariance embeds Sigma0.  Returns (mask as int, V as float64 [B, 12] numpy array or None)."""
    m = measurement_mask(mask, so3)
    if V is None:
        if m:
            raise ValueError("V is needed: mask %#05x measures something" % m)
        return m, None
    a = np.asarray(V.detach().cpu().numpy() if isinstance(V, torch.Tensor) else V, dtype=np.float64)
    sizes = (12, 6) if so3 else (12,)
    if a.ndim not in (1, 2) or a.shape[-1] not in sizes or (a.ndim == 2 and a.shape[0] != B):
        raise ValueError("V has shape %s, expected (%s) or (%d, %s)" % (tuple(a.shape), " or ".join(map(str, sizes)), B,
                                                                      " or ".join(map(str, sizes))))
    a = np.broadcast_to(a, (B, a.shape[-1]))
    if a.shape[-1] != 12:
        full = np.zeros((B, 12))
        full[:, _SO3_COORDS] = a
        a = full
    meas = np.array([(m >> j) & 1 for j in range(12)], dtype=bool)
    if not np.all(np.isfinite(a[:, meas])) or np.any(a[:, meas] <= 0.0):
        raise ValueError("V must be finite and positive on every measured coordinate")
    return m, np.ascontiguousarray(np.where(meas[None, :], a, 0.0))


@dataclass
class MPCResult:
    """`steps` closed-loop receding-horizon steps of B trajectories (BatchedTrackingILQR.mpc)."""
    xs_q: torch.Tensor     # [B, steps+1, 4, 4] closed-loop states: x0, then the plant state after every step
    xs_xi: torch.Tensor    # [B, steps+1, 6]
    us: torch.Tensor       # [B, steps, m] the applied inputs u*_0 of every step
    J: torch.Tensor        # [B] closed-loop cost: the sum of the stage costs l(x_t, u_t) against each step's window
    iters: torch.Tensor    # [B, steps] int32: iterations of each step's solve
    status: torch.Tensor   # [B, steps] int32: its status
    n_sat: Optional[torch.Tensor] = None  # [B, steps] int32 (mpc(u_lb=, u_ub=)): the inputs of each step the box moved
    n_rate: Optional[torch.Tensor] = None  # [B, steps] int32 (mpc(act_*=)): the inputs of each step the rate limit moved
    # mpc(lb=, ub=, obstacles=, obstacle_paths=): the planner's constraints
    max_violation: Optional[torch.Tensor] = None  # [B, steps] the largest g of each step's last plan (tolg_al_mpc_step)
    mu: Optional[torch.Tensor] = None             # [B] the penalty the loop ended with
    # ... with spheres: min_k |t_s - c_k(s)| - r_k(s) of the realised states at their world knots (negative: inside one)
    clearance: Optional[torch.Tensor] = None      # [B, steps+1]
    # mpc(pose_constraints=, pose_paths=): min_k pose_margin of the realised states at their world knots (negative: outside a cone)
    pose_margin: Optional[torch.Tensor] = None    # [B, steps+1]
    # mpc(meas_*=, est_*=): the loop on an estimate.  xs_q, xs_xi, J, clearance and pose_margin above are then those of the TRUE
    # states (the rule of policy_rollout_estimated: reports on the true state, never on the estimate); these are the filter's
    est_q: Optional[torch.Tensor] = None    # [B, steps+1, 4, 4] the posterior estimates, one per world knot
    est_xi: Optional[torch.Tensor] = None   # [B, steps+1, 6]
    est_var: Optional[torch.Tensor] = None  # [B, steps+1, 12] diag P^+
    innov: Optional[torch.Tensor] = None    # [B, steps+1, 12] the residuals r (0 on unmeasured coordinates)


MPC_EST_ACT = ("mpc: the estimated loop (meas_* / est_*) does not take an actuator model (act_tau / act_rate / act_delay): "
               "output feedback behind an actuator is out of scope, as it is for policy_rollout_estimated")


def check_owned(name, t, shapes, device):
    """A caller-owned in/out argument of mpc_measure / mpc_advance_estimated (act_state is the precedent): a contiguous
    float64 tensor on `device` of one of `shapes`; ValueError otherwise.  Returns t."""
    if (not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) not in [tuple(s) for s in shapes] or
            t.device != torch.device(device) or not t.is_contiguous()):
        raise ValueError("%s must be a contiguous float64 tensor of shape %s on %s"
                         % (name, " or ".join(str(tuple(s)) for s in shapes), device))
    return t


def check_mpc_estimated(B, steps, so3, meas_mask=None, meas_V=None, meas_noise=None, est_Sigma0=None, est_W=None, est_dx0=None,
                        actuated=False):
    """The six keywords of mpc()'s estimated loop checked on the host; ValueError before anything reaches the device.
    meas_mask / meas_V: check_measurement's (None: nothing is measured); meas_noise [B, steps+1, 12], est_dx0 [B, 12]: finite,
    None = 0 (the SO3 family: zero on coordinates 3..5 and 9..11); est_Sigma0 [12, 12] or [B, 12, 12], est_W [6, 6] or [B, 6, 6]:
    check_covariance's, None = 0.  actuated: the call also names an actuator model, which the estimated loop refuses.
    Returns (mask int, V [B, 12] or None, meas_noise [steps+1, B, 12] step-major or None, Sigma0 [B, 12, 12] (zeros for None),
    W [B, 6, 6] or None, dx0 [B, 12] or None), float64 numpy arrays."""
    if actuated:
        raise ValueError(MPC_EST_ACT)
    m, V = check_measurement(0 if meas_mask is None else meas_mask, meas_V, B, so3=so3)
    unused = [3, 4, 5, 9, 10, 11]
    n = None
    if meas_noise is not None:
        n = _checked("meas_noise", meas_noise, (B, steps + 1, 12), finite=True)
        if so3 and np.any(n[..., unused] != 0.0):
            raise ValueError("meas_noise: the SO3 family has no translation or linear velocity, coordinates 3..5 and 9..11 are 0")
        n = np.ascontiguousarray(n.transpose(1, 0, 2))  # step t: one contiguous [B, 12]
    S0 = np.zeros((B, 12, 12)) if est_Sigma0 is None else \
        check_covariance("est_Sigma0", est_Sigma0, B, 12, (6, _SO3_COORDS) if so3 else None)
    W = None if est_W is None else check_covariance("est_W", est_W, B, 6, (3, [0, 1, 2]) if so3 else None)
    d = None
    if est_dx0 is not None:
        d = _checked("est_dx0", est_dx0, (B, 12), finite=True)
        if so3 and np.any(d[:, unused] != 0.0):
            raise ValueError("est_dx0: the SO3 family has no translation or linear velocity, coordinates 3..5 and 9..11 are 0")
    return m, V, n, S0, W, d


def perturbed_state(x_q, x_xi, dx):
    """x (+) dx on the host, the right perturbation of the C ABI: x_q [B, 4, 4] Exp(dx[:, :6]) in the twist order [omega, v],
    x_xi + dx[:, 6:].  numpy in, numpy out."""
    x_q, x_xi, dx = (np.asarray(a, dtype=np.float64) for a in (x_q, x_xi, dx))
    out = np.empty((x_q.shape[0], 4, 4))
    for b in range(x_q.shape[0]):
        w, v = dx[b, :3], dx[b, 3:6]
        th = float(np.linalg.norm(w))
        Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        if th < 1e-6:
            a, bb, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
        else:
            a, bb, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        E = np.eye(4)
        E[:3, :3] = np.eye(3) + a * Wx + bb * Wx @ Wx
        E[:3, 3] = (np.eye(3) + bb * Wx + c * Wx @ Wx) @ v
        out[b] = x_q[b].reshape(4, 4) @ E
    return out, x_xi + dx[:, 6:]


def check_box(u_lb, u_ub, B, m, so3=False):
    """An actuator box checked on the host: u_lb, u_ub of shape [m] (every trajectory the same) or [B, m]; -inf / +inf mean
    no limit, NaN is refused, and lb <= ub must hold in every entry; ValueError otherwise, before anything reaches the device.
    so3: the problem is of the SO3 family (m = 6 with inputs 3..5 unused and zero) and the bounds may also be [3] or [B, 3], the
    unused rows then filled with -inf / +inf.  Returns (lb, ub) as float64 [B, m] numpy arrays."""
    out = []
    for name, a, fill in (("u_lb", u_lb, -np.inf), ("u_ub", u_ub, np.inf)):
        if a is None:
            raise ValueError("u_lb and u_ub come together: %s is missing" % name)
        a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
        sizes = (m, 3) if so3 else (m,)
        if a.ndim not in (1, 2) or a.shape[-1] not in sizes or (a.ndim == 2 and a.shape[0] != B):
            raise ValueError("%s has shape %s, expected (%s) or (%d, %s)" % (name, tuple(a.shape), " or ".join(map(str, sizes)),
                                                                          B, " or ".join(map(str, sizes))))
        if np.isnan(a).any():
            raise ValueError("%s must not hold NaN (-inf / +inf mean no limit)" % name)
        a = np.broadcast_to(a, (B, a.shape[-1]))
        if a.shape[-1] != m:
            a = np.concatenate([a, np.full((B, m - a.shape[-1]), fill)], axis=1)
        out.append(np.ascontiguousarray(a))
    if np.any(out[0] > out[1]):
        raise ValueError("u_lb must not exceed u_ub")
    if so3 and (np.any(out[0][:, 3:] > 0.0) or np.any(out[1][:, 3:] < 0.0)):
        raise ValueError("inputs 3..5 of the %s are unused and zero: their bounds must contain 0" % "SO3 family")
    return out[0], out[1]


def check_input_box(lb, ub, B, N, m):
    """The planner's input box (set_al, al_fit_batch, plan_fleet, mpc) checked on the host, ValueError before anything
    reaches the device: lb, ub of one shape, [m] (every trajectory and knot the same: tolg_set_al), [B, m] (a box per
    trajectory) or [B, N, m] (per knot: tolg_set_al_box); finite -- the augmented-Lagrangian terms multiply lambda by g = lb -
    u, and an infinite bound makes that NaN: a missing limit is a wide finite one, unlike the actuator box of check_box --
    and lb <= ub in every entry.  Returns (lb, ub) as contiguous float64 numpy arrays of the shape given."""
    out = []
    for name, a in (("lb", lb), ("ub", ub)):
        if a is None:
            raise ValueError("lb and ub come together: %s is missing" % name)
        a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
        if tuple(a.shape) not in ((m,), (B, m), (B, N, m)):
            raise ValueError("%s has shape %s, expected (%d), (%d, %d) or (%d, %d, %d)" % (name, tuple(a.shape), m, B, m, B, N, m))
        if not np.all(np.isfinite(a)):
            raise ValueError("%s must be finite (a missing limit is a wide finite one: lambda * g with an infinite g is NaN)" % name)
        out.append(np.ascontiguousarray(a))
    if out[0].shape != out[1].shape:
        raise ValueError("lb %s and ub %s must have the same shape" % (out[0].shape, out[1].shape))
    if np.any(out[0] > out[1]):
        raise ValueError("lb must not exceed ub")
    return out[0], out[1]


def check_actuator(u_lb, u_ub, tau, rate, delay, u_init, B, m, dt, so3=False):
    """An actuator model (include/tolg.h, tolg_actuator) checked and converted on the host, ValueError before anything reaches
    the device.  u_lb / u_ub: the box of check_box, both or neither (None).  tau: the lag's time constant in seconds, [m] or
    [B, m] (or one number for every input, as rate), finite and >= 0 with 0 meaning no lag, converted to beta = exp(-dt / tau) (tau = 0 gives beta = 0.0 exactly).
    rate: the slew limit in units per second, > 0 with inf allowed, converted to du = rate * dt per knot.  delay: whole knots,
    an int in 0..4 (TOLG_MAX_ACT_DELAY).  u_init [m] or [B, m], finite: the input the actuator holds before the first knot
    (None: u*_0).  so3: as check_box -- tau, rate and u_init may also be [3] or [B, 3] (rows 3..5 filled with 0, inf and 0), the
    box rows 3..5 must contain 0 and u_init rows 3..5 equal it.
    Returns (lb, ub, beta, du, u_init, delay): float64 [B, m] numpy arrays, None for what was not given."""
    if not (np.ndim(dt) == 0 and np.isfinite(dt) and dt > 0):
        raise ValueError("dt must be a positive number")
    if isinstance(delay, (bool, np.bool_)) or not isinstance(delay, (int, np.integer)):
        raise ValueError("act_delay must be an int (whole knots), got %r" % (delay,))
    if not 0 <= int(delay) <= _capi.MAX_ACT_DELAY:
        raise ValueError("act_delay %d outside 0..%d" % (delay, _capi.MAX_ACT_DELAY))
    lb = ub = None
    if u_lb is not None or u_ub is not None:
        lb, ub = (np.array(a) for a in check_box(u_lb, u_ub, B, m, so3=so3))  # (copies: a broadcast view is read-only)

    def rows(name, a, fill, scalar=True):
        a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
        if scalar and a.ndim == 0:  # one value for every input
            a = np.full(m, float(a))
        sizes = (m, 3) if so3 else (m,)
        if a.ndim not in (1, 2) or a.shape[-1] not in sizes or (a.ndim == 2 and a.shape[0] != B):
            raise ValueError("%s has shape %s, expected (%s) or (%d, %s)" % (name, tuple(a.shape), " or ".join(map(str, sizes)),
                                                                          B, " or ".join(map(str, sizes))))
        if np.isnan(a).any():
            raise ValueError("%s must not hold NaN" % name)
        a = np.broadcast_to(a, (B, a.shape[-1]))
        if a.shape[-1] != m:
            a = np.concatenate([a, np.full((B, m - a.shape[-1]), fill)], axis=1)
        return np.array(a, order="C")  # (a copy: a broadcast view is read-only)

    beta = du = ui = None
    if tau is not None:
        t = rows("act_tau", tau, 0.0)
        if not np.all(np.isfinite(t)) or np.any(t < 0.0):
            raise ValueError("act_tau must be finite and >= 0 (seconds; 0: no lag)")
        with np.errstate(divide="ignore"):
            beta = np.where(t > 0.0, np.exp(-float(dt) / np.where(t > 0.0, t, 1.0)), 0.0)
    if rate is not None:
        r = rows("act_rate", rate, np.inf)
        if np.any(r <= 0.0):
            raise ValueError("act_rate must be > 0 (units per second; inf: no limit)")
        du = r * float(dt)
    if u_init is not None:
        ui = rows("act_u_init", u_init, 0.0, scalar=False)
        if not np.all(np.isfinite(ui)):
            raise ValueError("act_u_init must be finite")
        if so3 and np.any(ui[:, 3:] != 0.0):
            raise ValueError("inputs 3..5 of the SO3 family are unused and zero: act_u_init must be 0 there")
    return lb, ub, beta, du, ui, int(delay)


def actuator_state(us0, delay):
    """The initial actuator state of mpc_advance(act_state=) from u*_0 = us0 [B, m]: [B, 1 + delay, m], row 0 (the last applied
    input) and the `delay` pending commands all u*_0 -- an actuator at rest on the first command.  A torch tensor gives a new
    contiguous tensor on its device, anything else a float64 numpy array."""
    if isinstance(delay, (bool, np.bool_)) or not isinstance(delay, (int, np.integer)) or not 0 <= delay <= _capi.MAX_ACT_DELAY:
        raise ValueError("delay must be an int in 0..%d" % _capi.MAX_ACT_DELAY)
    if isinstance(us0, torch.Tensor):
        if us0.ndim != 2:
            raise ValueError("us0 has shape %s, expected (B, m)" % (tuple(us0.shape),))
        return us0.to(torch.float64)[:, None, :].repeat(1, 1 + int(delay), 1).contiguous()
    a = np.asarray(us0, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("us0 has shape %s, expected (B, m)" % (tuple(a.shape),))
    return np.ascontiguousarray(np.repeat(a[:, None, :], 1 + int(delay), axis=1))


# The kinds of a constraint slot (TOLG_OBS_*, include/tolg.h has the table of rows and clearances), by number or by name
OBSTACLE_KINDS = {"sphere": _capi.OBS_KEEP_OUT, "keep_in": _capi.OBS_KEEP_IN, "half_space": _capi.OBS_HALF_SPACE,
                  "column": _capi.OBS_COLUMN_Z}


def check_kinds(kinds, K):
    """The kinds of K slots as a tuple of ints 0..3: a length-K sequence of ints or of OBSTACLE_KINDS names; None: K keep-out
    spheres.  ValueError for another length or an unknown kind."""
    if kinds is None:
        return (0,) * int(K)
    kinds = list(kinds)
    if len(kinds) != int(K):
        raise ValueError("kinds has %d entries, expected one per slot: K = %d" % (len(kinds), K))
    out = []
    for k in kinds:
        if isinstance(k, str):
            if k not in OBSTACLE_KINDS:
                raise ValueError("unknown obstacle kind %r, expected one of %s" % (k, sorted(OBSTACLE_KINDS)))
            out.append(OBSTACLE_KINDS[k])
        elif isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 0 <= int(k) <= 3:
            out.append(int(k))
        else:
            raise ValueError("unknown obstacle kind %r, expected 0..3 or one of %s" % (k, sorted(OBSTACLE_KINDS)))
    return tuple(out)


def check_kind_geometry(name, a, kinds):
    """The fields of every slot under its kind, a [..., K, 4] numpy or torch: a positive radius in the spheres and the column,
    a unit normal (||n| - 1| <= 1e-9, never rescaled: the offset is measured along it) in a half-space, whose offset may be
    any finite number.  ValueError otherwise."""
    for k, kd in enumerate(kinds):
        s = a[..., k, :]
        if kd == _capi.OBS_HALF_SPACE:
            n2 = (s[..., :3] ** 2).sum(-1)
            if bool((abs(n2 ** 0.5 - 1.0) > 1e-9).any()):
                raise ValueError("%s: slot %d is a half-space and needs a unit normal (nx, ny, nz), | |n| - 1 | <= 1e-9" % (name, k))
        elif bool((s[..., 3] <= 0.0).any()):
            raise ValueError("%s: every radius must be positive (slot %d)" % (name, k))


def kind_clearance(t, geo, kinds):
    """The clearance of positions t [..., 3] from slots geo [..., K, 4] (shapes that broadcast) under `kinds`, [..., K], numpy
    or torch alike: >= 0 inside the allowed set (tolg_policy_rollout_limited's d_clear is its minimum)."""
    out = []
    for k, kd in enumerate(kinds):
        f = geo[..., k, :]
        if kd == _capi.OBS_HALF_SPACE:
            out.append(f[..., 3] - (f[..., :3] * t).sum(-1))
            continue
        d = t - f[..., :3]
        d2 = (d[..., :2] ** 2).sum(-1) if kd == _capi.OBS_COLUMN_Z else (d ** 2).sum(-1)
        c = d2 ** 0.5 - f[..., 3]
        out.append(-c if kd == _capi.OBS_KEEP_IN else c)
    return (torch if isinstance(out[0], torch.Tensor) else np).stack(out, -1)


# The kinds of a pose-constraint slot (TOLG_POSE_*, include/tolg.h has the table of rows, gradients and margins): the second
# slot family, beside OBSTACLE_KINDS and apart from it
POSE_CONSTRAINT_KINDS = {"tilt_cone": _capi.POSE_TILT_CONE, "view_cone": _capi.POSE_VIEW_CONE}


def check_pose_kinds(kinds, K):
    """The kinds of K pose slots as a tuple of ints 0..1: a length-K sequence of ints or of POSE_CONSTRAINT_KINDS names.
    ValueError for None (a pose slot has no default kind), another length or an unknown kind."""
    if kinds is None:
        raise ValueError("pose constraints need their kinds: one of %s per slot" % sorted(POSE_CONSTRAINT_KINDS))
    kinds = list(kinds)
    if len(kinds) != int(K):
        raise ValueError("pose kinds has %d entries, expected one per slot: K = %d" % (len(kinds), K))
    out = []
    for k in kinds:
        if isinstance(k, str) and k in POSE_CONSTRAINT_KINDS:
            out.append(POSE_CONSTRAINT_KINDS[k])
        elif isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 0 <= int(k) <= 1:
            out.append(int(k))
        else:
            raise ValueError("unknown pose constraint kind %r, expected 0..1 or one of %s" % (k, sorted(POSE_CONSTRAINT_KINDS)))
    return tuple(out)


def check_pose_geometry(name, a, kinds):
    """The fields of every pose slot under its kind, a [..., K, 4] numpy or torch: a tilt cone needs a unit world axis (nx, ny,
    nz), ||n| - 1| <= 1e-9 (never rescaled), a view cone a finite target (px, py, pz); both -1 < c < 1, the cosine of the
    largest tilt / of the half angle.  ValueError otherwise."""
    for k, kd in enumerate(kinds):
        s = a[..., k, :]
        if not bool(((s == s) & (abs(s) != float("inf"))).all()):
            raise ValueError("%s must be finite (slot %d)" % (name, k))
        if kd == _capi.POSE_TILT_CONE:
            n2 = (s[..., :3] ** 2).sum(-1)
            if bool((abs(n2 ** 0.5 - 1.0) > 1e-9).any()):
                raise ValueError("%s: slot %d is a tilt cone and needs a unit axis (nx, ny, nz), | |n| - 1 | <= 1e-9" % (name, k))
        if not bool(((s[..., 3] > -1.0) & (s[..., 3] < 1.0)).all()):
            raise ValueError("%s: slot %d needs -1 < c < 1, the cosine of its angle" % (name, k))


def pose_margin(xs_q, slots, kinds):
    """The margins of poses xs_q [..., 4, 4] under pose slots [..., K, 4] (leading shapes that broadcast against those of xs_q:
    [K, 4], [B, K, 4], [B, N+1, K, 4], with a sample axis [B, 1, N+1, K, 4]) of `kinds`, [..., K], numpy or torch alike: >= 0
    inside the allowed set.  Tilt cone n^T R e3 - c: the cosine of the tilt above that of the limit; view cone e1^T b / |b| - c
    with b = R^T (p - t).  On the states of policy_rollout(trajectories=True) this is the Monte-Carlo check of a limit under
    noise."""
    kinds = check_pose_kinds(kinds, slots.shape[-2])
    R, t = xs_q[..., :3, :3], xs_q[..., :3, 3]
    out = []
    for k, kd in enumerate(kinds):
        f = slots[..., k, :]
        if kd == _capi.POSE_TILT_CONE:
            out.append((f[..., :3] * R[..., :, 2]).sum(-1) - f[..., 3])
            continue
        d = f[..., :3] - t
        b = (R * d[..., :, None]).sum(-2)   # R^T d
        out.append(b[..., 0] / (b ** 2).sum(-1) ** 0.5 - f[..., 3])
    return (torch if isinstance(out[0], torch.Tensor) else np).stack(out, -1)


def _min_first_knot(m):
    """min over the knot and slot axes of m [..., N+1, K] and the first knot that attains it, under the kernels' order rule:
    strict <, knots ascending, slots ascending; a NaN is passed over; +inf and knot 0 where no entry is a number."""
    np_ = not isinstance(m, torch.Tensor)
    inf = float("inf")
    m = (np.where(np.isnan(m), inf, m) if np_ else torch.where(torch.isnan(m), torch.full_like(m, inf), m))
    per_knot = m.min(-1) if np_ else m.amin(-1)           # [..., N+1]
    # argmin returns the first index of the minimum in numpy and in torch alike
    knot = per_knot.argmin(-1)
    return (per_knot.min(-1) if np_ else per_knot.amin(-1)), (knot.astype(np.int32) if np_ else knot.to(torch.int32)), per_knot


def rollout_margins(xs_q, obstacles=None, kinds=None, pose_slots=None, pose_kinds=None):
    """The margin report of the sampled closed loops from stored trajectories, the definition tolg_policy_rollout_margins and
    tolg_policy_rollout_estimated_limited are tested against and the fallback for whoever holds trajectories already: xs_q
    [B, S, N+1, 4, 4] (policy_rollout(trajectories=True).xs_q), numpy or torch alike.  obstacles [K, 4], [B, K, 4] or
    [B, N+1, K, 4] of `kinds` (check_kinds; None: keep-out spheres) and / or pose_slots of the same three shapes of
    `pose_kinds` (check_pose_kinds); a family not given is not reported.  Returns a dict with, per family given,
      clearance, clearance_knot [B, S]        min over knots and slots of kind_clearance, and the first knot that attains it
      pose_margin, pose_margin_knot [B, S]    the same of pose_margin()
      viol_pos, viol_pose [B, N+1] int32      per knot, the samples whose minimum over the slots is < 0 there
    under the kernels' order rule: strict <, knots then slots ascending, a NaN passed over (and no violation), +inf and knot 0
    where no margin is a number."""
    if xs_q.ndim != 5 or tuple(xs_q.shape[-2:]) != (4, 4):
        raise ValueError("rollout_margins: xs_q has shape %s, expected (B, S, N+1, 4, 4)" % (tuple(xs_q.shape),))
    if obstacles is None and pose_slots is None:
        raise ValueError("rollout_margins needs obstacles or pose_slots")
    B, N1 = xs_q.shape[0], xs_q.shape[2]
    is_t = isinstance(xs_q, torch.Tensor)

    def slots_for(name, a):
        a = (torch.as_tensor(a, dtype=xs_q.dtype, device=xs_q.device) if is_t
             else np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64))
        ok = a.ndim in (2, 3, 4) and a.shape[-1] == 4 and (a.ndim == 2 or a.shape[0] == B) and (a.ndim < 4 or a.shape[1] == N1)
        if not ok:
            raise ValueError("rollout_margins: %s has shape %s, expected (K, 4), (%d, K, 4) or (%d, %d, K, 4)"
                             % (name, tuple(a.shape), B, B, N1))
        # against the sample and knot axes of xs_q: [B or 1, 1, N+1 or 1, K, 4]
        return a if a.ndim == 2 else (a[:, None, None] if a.ndim == 3 else a[:, None])

    out = {}
    count = lambda v: (v.sum(1).to(torch.int32) if is_t else v.sum(1).astype(np.int32))  # noqa: E731
    if obstacles is not None:
        o = slots_for("obstacles", obstacles)
        c = kind_clearance(xs_q[..., :3, 3], o, check_kinds(kinds, o.shape[-2]))
        out["clearance"], out["clearance_knot"], per_knot = _min_first_knot(c)
        out["viol_pos"] = count(per_knot < 0.0)
    if pose_slots is not None:
        o = slots_for("pose_slots", pose_slots)
        m = pose_margin(xs_q, o, pose_kinds)
        out["pose_margin"], out["pose_margin_knot"], per_knot = _min_first_knot(m)
        out["viol_pose"] = count(per_knot < 0.0)
    return out


def inflate_obstacles(obstacles, xs_q, pos_cov, kappa, kinds=None):
    """Keep-out spheres with a margin for the closed-loop spread: obstacles [K, 4], [B, K, 4] or [B, N+1, K, 4] rows (cx, cy,
    cz, r), xs_q [B, N+1, 4, 4] the nominal plan, pos_cov [B, N+1, 3, 3] its position covariance (policy_covariance().pos_cov).
    Returns [B, N+1, K, 4] (numpy) with the radii r_ik + kappa sqrt(n_ik^T pos_cov_i n_ik), n_ik the unit vector from c_ik to
    the nominal position t_i: kappa standard deviations of the position along the line to the sphere, a radius per knot,
    which is what al_fit_batch(obstacles=...) takes.
    kinds (check_kinds; None: all keep-out spheres): with sigma = sqrt(n^T pos_cov n) a keep-in sphere shrinks, r - kappa sigma
    (ValueError where a radius stops being positive); a half-space moves in along its own normal n, o - kappa sigma; a column
    grows, r + kappa sigma, with n the horizontal unit vector from its axis to t_i."""
    host = lambda a: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)  # noqa: E731
    t, cov, o = host(xs_q)[..., :3, 3], host(pos_cov), host(obstacles)
    B, N1 = t.shape[:2]
    if o.ndim < 4:
        o = np.broadcast_to(o if o.ndim == 2 else o[:, None], (B, N1) + o.shape[-2:])
    if o.shape[:2] != (B, N1) or o.shape[-1] != 4 or cov.shape != (B, N1, 3, 3):
        raise ValueError("inflate_obstacles: obstacles %s and pos_cov %s do not fit xs_q [%d, %d, 4, 4]" % (o.shape, cov.shape, B, N1))
    kd = np.asarray(check_kinds(kinds, o.shape[2]))
    n = t[:, :, None, :] - o[..., :3]
    n[..., 2] = np.where(kd == _capi.OBS_COLUMN_Z, 0.0, n[..., 2])
    n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-300)
    n = np.where((kd == _capi.OBS_HALF_SPACE)[:, None], o[..., :3], n)
    var = np.einsum("bika,biac,bikc->bik", n, cov, n)
    out = o.copy()
    sign = np.where((kd == _capi.OBS_KEEP_IN) | (kd == _capi.OBS_HALF_SPACE), -1.0, 1.0)
    out[..., 3] += sign * (float(kappa) * np.sqrt(np.maximum(var, 0.0)))
    if np.any(out[..., kd == _capi.OBS_KEEP_IN, 3] <= 0.0):
        raise ValueError("inflate_obstacles: a keep-in radius is not positive once kappa sigma is taken off")
    return out


def tighten_pose_constraints(slots, kinds, xs_q, Sigma, kappa):
    """Pose slots with a margin for the closed-loop spread, the pose family's inflate_obstacles: slots [K, 4], [B, K, 4] or
    [B, N+1, K, 4] of `kinds` (check_pose_kinds), xs_q [B, N+1, 4, 4] the nominal plan, Sigma [B, N+1, 12, 12] its covariance
    (policy_covariance(full=True).Sigma), whose pose block Sigma[..., :6, :6] is in the error coordinates X Exp(delta), delta =
    [omega, v], of the rows' gradients g_x = [g_omega, g_v] (include/tolg.h has the table).  With sigma_ik = sqrt(g_x^T
    Sigma_pose g_x) at the nominal pose -- one standard deviation of the row to first order -- a tilt cone gets the cosine c +
    kappa sigma, a view cone c + kappa sigma / |b|: its row is |b| times the gap of the cosines, b = R^T (p - t), so that is
    kappa standard deviations of the margin (exactly so, to first order, for a pose on the cone; off it the row's gradient and
    the margin's differ by (c - cos) along the line of sight).  Returns [B, N+1, K, 4] (numpy), the per-knot form
    al_fit_batch(pose_constraints=) and mpc(pose_paths=) take.  ValueError where a cosine reaches 1: no cone is left."""
    host = lambda a: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)  # noqa: E731
    x, cov, o = host(xs_q), host(Sigma), host(slots)
    if x.ndim != 4 or x.shape[-2:] != (4, 4):
        raise ValueError("tighten_pose_constraints: xs_q has shape %s, expected (B, N+1, 4, 4)" % (x.shape,))
    B, N1 = x.shape[:2]
    if o.ndim in (2, 3):
        o = np.broadcast_to(o if o.ndim == 2 else o[:, None], (B, N1) + o.shape[-2:])
    if o.ndim != 4 or o.shape[:2] != (B, N1) or o.shape[-1] != 4 or cov.shape != (B, N1, 12, 12):
        raise ValueError("tighten_pose_constraints: slots %s and Sigma %s do not fit xs_q [%d, %d, 4, 4]" % (o.shape, cov.shape, B, N1))
    kd = check_pose_kinds(kinds, o.shape[2])
    R, t = x[..., :3, :3], x[..., :3, 3]
    e1, e3 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    out = o.copy()
    for k, kind in enumerate(kd):
        f, c = o[:, :, k, :3], o[:, :, k, 3]
        if kind == _capi.POSE_TILT_CONE:
            a = np.einsum("biac,bia->bic", R, f)                    # R^T n
            gx, scale = np.concatenate([np.cross(a, e3), np.zeros_like(a)], axis=-1), 1.0
        else:
            b = np.einsum("biac,bia->bic", R, f - t)                # R^T (p - t)
            nb = np.linalg.norm(b, axis=-1)
            gx, scale = np.concatenate([np.cross(b, e1), e1 - (c / nb)[..., None] * b], axis=-1), 1.0 / nb
        var = np.einsum("bia,biac,bic->bi", gx, cov[:, :, :6, :6], gx)
        out[:, :, k, 3] = c + float(kappa) * np.sqrt(np.maximum(var, 0.0)) * scale
    if np.any(out[..., 3] >= 1.0):
        raise ValueError("tighten_pose_constraints: a cosine reaches 1 once kappa sigma is added: no cone is left")
    return out


def tighten_input_box(lb, ub, var_u, kappa):
    """The input box with a margin for the closed-loop spread, the input half of inflate_obstacles and
    tighten_pose_constraints: lb, ub [m], [B, m] or [B, N, m], var_u [B, N, m] the variance of the held policy's inputs
    (policy_covariance().var_u).  Returns (lb + kappa sqrt(var_u), ub - kappa sqrt(var_u)), [B, N, m] each (numpy): kappa
    standard deviations of room for the feedback on either side at every knot, the per-knot form al_fit_batch(lb=, ub=) and
    mpc(lb=, ub=) take.  ValueError where the box would become empty."""
    host = lambda a: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)  # noqa: E731
    var = host(var_u)
    if var.ndim != 3:
        raise ValueError("tighten_input_box: var_u has shape %s, expected (B, N, m)" % (var.shape,))
    B, N, m = var.shape
    lo, hi = check_input_box(lb, ub, B, N, m)
    if not np.all(np.isfinite(var)) or np.any(var < 0.0) or not np.isfinite(float(kappa)) or float(kappa) < 0.0:
        raise ValueError("tighten_input_box: var_u must be finite and not negative, kappa finite and not negative")
    grow = lambda a: a if a.ndim == 3 else np.broadcast_to(a if a.ndim == 1 else a[:, None], (B, N, m))  # noqa: E731
    s = float(kappa) * np.sqrt(var)
    lo, hi = grow(lo) + s, grow(hi) - s
    if np.any(lo > hi):
        raise ValueError("tighten_input_box: the box is empty once kappa sigma is taken off both sides")
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


def mpc_window_index(t0, t, N, T):
    """Knot of the path that knot i of step t's window tracks (tolg_set_ref_windows): min(t0[b] + t + i, T), [B, N+1]."""
    t0 = np.asarray(t0, dtype=np.int64).reshape(-1)
    return np.clip(t0[:, None] + int(t) + np.arange(N + 1)[None, :], 0, int(T))


def mpc_shift(xs, us, x_next, x_tail):
    """The warm start tolg_mpc_advance builds, on the host: xs [B, N+1, ...], us [B, N, m] a step's solution, x_next [B, ...]
    the plant's next state, x_tail [B, ...] = f(x*_N, u*_{N-1}).  Returns (xs_warm, us_warm): xs_warm[0] = x_next,
    xs_warm[i] = xs[i+1] (1 <= i < N), xs_warm[N] = x_tail; us_warm[i] = us[i+1], the last input held."""
    xs, us = np.asarray(xs), np.asarray(us)
    xs_w = np.concatenate([np.asarray(x_next)[:, None], xs[:, 2:], np.asarray(x_tail)[:, None]], axis=1)
    us_w = np.concatenate([us[:, 1:], us[:, -1:]], axis=1)
    return xs_w, us_w


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _checked(name, a, shape, finite=False):
    """The host-side check of a batch input: `a` (numpy, torch or nested sequences) has `shape` (None: any extent) and, with
    finite=True, only finite values; ValueError otherwise, before anything reaches the device.  Returns `a` as given (nested
    sequences as a float64 array), or with finite=True as a float64 numpy array (a device tensor is read back)."""
    if finite:
        a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    elif not hasattr(a, "shape"):
        a = np.asarray(a, dtype=np.float64)
    s = tuple(a.shape)
    if len(s) != len(shape) or any(n is not None and n != k for n, k in zip(shape, s)):
        raise ValueError("%s has shape %s, expected (%s)" % (name, s, ", ".join("*" if n is None else str(n) for n in shape)))
    if finite and not np.all(np.isfinite(a)):
        raise ValueError("%s must be finite" % name)
    return a


# What a C call does to the held policy (include/tolg.h): "clear" before it runs (so also when it fails), "hold" the batch
# of the call once it has succeeded.  gains / policy_rollout / mpc_advance need one held.
_POLICY = {"tolg_solve_begin": "clear", "tolg_solve_begin_warm": "clear", "tolg_eval_knot": "clear",
           "tolg_solve_batch": "clear hold", "tolg_linearize_backward": "clear hold", "tolg_solve_end": "hold",
           "tolg_set_al_obstacles": "", "tolg_set_al_obstacles_moving": "",
           "tolg_al_update_state": "", "tolg_al_mpc_step": "", "tolg_al_mpc_step_pose": "",
           "tolg_set_al_obstacle_windows": "", "tolg_set_al_obstacle_kinds": "",
           "tolg_set_al_pose_constraints": "", "tolg_set_al_pose_constraint_windows": "",
           "tolg_policy_rollout_margins": "", "tolg_policy_rollout_estimated_limited": ""}  # (the last eleven leave it: listed for completeness)
# A setter's detach call (BatchedTrackingILQR._detach): its arguments behind the handle with the source pointer null, the
# stream's place included.  tolg_set_al_obstacles detaches the per-knot form too.
_DETACH = {"tolg_set_refs": (0, None, None, None, 0, None), "tolg_set_weights": (0, None, None, None, None, 0, None),
           "tolg_set_pose_schedule": (0, None, None, 0, None),
           "tolg_set_al_obstacles": (0, 0, None, None, None, None, 0, None), "tolg_set_al": (None, None, None, None),
           "tolg_set_al_pose_constraints": (0, 0, None, None, 0, None, None, None, 0, None),
           "tolg_set_plant": (0, 0, 0, None, None, None, 0, None)}


@dataclass
class _Batch:
    """A batch's inputs, checked and on the device (BatchedTrackingILQR._stage)."""
    B: int
    x_q: torch.Tensor     # [B, 16] the initial states (linearize_backward: [B, N+1, 16], whole trajectories)
    x_xi: torch.Tensor    # [B, 6] ([B, N+1, 6])
    us: torch.Tensor      # [B, N, m]
    refs: Optional[tuple] = None  # (q [B, N+1, 16], xi [B, N+1, 6]) per trajectory, or None: the problem's reference
    wts: Optional[tuple] = None   # diagonals (q [B, 12], p [B, 12], r [B, m]) per trajectory, or None: the problem's weights
    xs: Optional[tuple] = None    # warm-start shooting states (q [B, N+1, 16], xi [B, N+1, 6]), or None
    # the pose schedule on wts: the factors ([B, N+1, 6],), or staged windows (paths [B, T+1, 6], T, t0 or None, t), or None
    sched: Optional[tuple] = None


class BatchedTrackingILQR:
    """Batched iLQR_Tracking_SE3_MS / iLQR_Tracking_SE3 on one GPU (one process per GPU).

    The object owns a device workspace tensor (allocated once, here) and an opaque C handle; the
    solve calls allocate nothing inside the library."""

    def __init__(self, problem: TrackingProblem, max_batch: int, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the batched solver is HIP-only (there is no CPU fallback)")
        self.lib = _capi.load()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.problem = problem
        self.N, self.m = problem.N, problem.m
        self.max_batch = int(max_batch)
        self._policy_B = 0         # batch of the held policy, 0 = none (_POLICY)
        self._refs_set = self._wts_set = False  # the handle points at per-trajectory references / weights
        # the packed inputs the handle reads (_packed): per-trajectory references, weights and static spheres for max_batch
        # (x MAX_OBSTACLES), per-knot spheres and plant rows for the largest call so far
        self._refs_buf = self._wts_buf = self._obs_buf = self._obs_mov_buf = self._plant_buf = self._sched_buf = None
        self._sched_next = None    # set_pose_schedule_windows: the staged windows the next batch call takes (_Batch.sched)
        self._inflight = (None, None)  # the FitResult of the solve in flight; the inputs the stream may not have read (_hold)
        self._al = None            # the augmented-Lagrangian terms the handle points at (set_al)
        self._obs = None           # ... and the keep-out spheres (set_al_obstacles): (obstacles, lam, imu) on the device
        self._obs_kinds = ()       # ... with the kinds the handle holds for them (tolg_set_al_obstacle_kinds), one per slot
        self._pose = None          # ... and the pose constraints (set_al_pose_constraints): (slots, lam, imu, kinds)
        self._pose_buf = self._pose_knot_buf = None  # their packed geometry: static for max_batch, per knot for the largest call
        self._box_win = None       # set_al_box_windows: the gathered windows (lb, ub) [B, N, m] the handle reads in place
        p = _capi.Problem()
        p.kind, p.m, p.N, p.dt = _KIND[problem.kind], self.m, self.N, float(problem.dt)
        p.pend_mass, p.pend_length = float(problem.pend_mass), float(problem.pend_length)
        p.J[:] = list(np.asarray(problem.J, dtype=np.float64).reshape(36))
        p.Q[:] = list(np.asarray(problem.Q, dtype=np.float64).reshape(144))
        p.P[:] = list(np.asarray(problem.P, dtype=np.float64).reshape(144))
        Rm = np.zeros(36)
        Rm[: self.m * self.m] = np.asarray(problem.R, dtype=np.float64).reshape(-1)
        p.R[:] = list(Rm)
        self._p = p
        nbytes = self.lib.tolg_workspace_bytes(C.byref(p), self.max_batch)
        if nbytes == 0:
            raise ValueError("invalid problem description")
        self.workspace_bytes = int(nbytes)
        with torch.cuda.device(self.device):
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            off = (-self._ws.data_ptr()) % 256
            self._ws_ptr = self._ws.data_ptr() + off
            self._q_ref = torch.as_tensor(np.ascontiguousarray(problem.q_ref, dtype=np.float64).reshape(self.N + 1, 16),
                                          device=self.device)
            self._xi_ref = torch.as_tensor(np.ascontiguousarray(problem.xi_ref, dtype=np.float64).reshape(self.N + 1, 6),
                                           device=self.device)
            h = C.c_void_p()
            rc = self.lib.tolg_create(C.byref(p), _ptr(self._q_ref), _ptr(self._xi_ref), self.max_batch,
                                      C.c_void_p(self._ws_ptr), C.c_size_t(nbytes), self._stream(), C.byref(h))
        _capi.check(rc, "tolg_create")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            self.lib.tolg_destroy(h)
            self._h = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, fn, *args, stream=True, batch=0):
        """C entry point `fn` on the handle, checked.  stream=True: on the solver's device, its current stream appended as the
        last argument.  The held policy follows _POLICY; `batch` is the one a "hold" call leaves."""
        effect = _POLICY.get(fn, "")
        if "clear" in effect:
            self._policy_B = 0
        if stream:
            with torch.cuda.device(self.device):
                rc = getattr(self.lib, fn)(self._h, *args, self._stream())
        else:
            rc = getattr(self.lib, fn)(self._h, *args)
        _capi.check(rc, fn)
        if "hold" in effect:
            self._policy_B = int(batch)

    def _dev(self, a, shape):
        t = torch.as_tensor(a, dtype=torch.float64, device=self.device)
        return t.reshape(shape).contiguous()

    def _hold(self, inputs):
        """The one keep-alive: the device inputs of the last call, which the stream may not have read yet."""
        self._inflight = (self._inflight[0], inputs)

    def _packed(self, attr, nbytes_fn, *n, B=None):
        """The caller-owned buffer self.<attr> a setter packs into and the handle reads, of nbytes_fn(problem, B, *n) bytes (the
        setter's tolg_*_bytes).  B = None: for max_batch, allocated once (references, weights, static spheres); B given: for
        this call, kept and grown when a later call needs more (per-knot spheres, plants).  Returns (pointer, bytes)."""
        need = int(nbytes_fn(C.byref(self._p), self.max_batch if B is None else B, *n)) // 8
        buf = getattr(self, attr)
        if buf is None or buf.numel() < need:
            buf = torch.empty(need, dtype=torch.float64, device=self.device)
            setattr(self, attr, buf)
        return _ptr(buf), C.c_size_t(buf.numel() * 8)

    def _detach(self, fn):
        """Return the handle to what tolg_create left for setter `fn` (_DETACH).  On the solver's stream where the setter takes
        one: detaching the weights or the schedule writes the device constants in stream order."""
        if fn == "tolg_set_al":
            self._call(fn, *_DETACH[fn], stream=False)
        else:
            self._call(fn, *_DETACH[fn][:-1])

    def _check_refs(self, B, q_ref, xi_ref):
        """Per-trajectory references [B, N+1, 4, 4] / [B, N+1, 6], checked on the host: ValueError before anything reaches
        the device.  None when both are omitted (the problem's shared reference)."""
        if q_ref is None and xi_ref is None:
            return None
        if q_ref is None or xi_ref is None:
            raise ValueError("per-trajectory references need both q_ref and xi_ref")
        return _checked("q_ref", q_ref, (B, self.N + 1, 4, 4)), _checked("xi_ref", xi_ref, (B, self.N + 1, 6))

    def _check_weights(self, B, Q, P, R):
        """Per-trajectory cost weights Q [B, 12, 12], P [B, 12, 12], R [B, m, m] (numpy or torch, the fields of TrackingProblem
        per trajectory), checked on the host: ValueError before anything reaches the device for a wrong shape, an off-diagonal
        entry that is not zero, a negative or non-finite weight.  Returns the diagonals (q [B, 12], p [B, 12], r [B, m], float64
        numpy), or None when all three are omitted (the problem's shared weights)."""
        if Q is None and P is None and R is None:
            return None
        if Q is None or P is None or R is None:
            raise ValueError("per-trajectory weights need all three of Q, P and R")
        out = []
        for name, a, n in (("Q", Q, 12), ("P", P, 12), ("R", R, self.m)):
            a = _checked(name, a, (B, n, n), finite=True)
            d = np.diagonal(a, axis1=1, axis2=2)
            if np.any(a - d[:, :, None] * np.eye(n) != 0.0):
                raise ValueError("%s: per-trajectory weights must be diagonal (a non-zero off-diagonal entry)" % name)
            if np.any(d < 0.0):
                raise ValueError("%s: per-trajectory weights must not be negative" % name)
            out.append(np.ascontiguousarray(d))
        return tuple(out)

    def _check_pose_scale(self, B, pose_scale):
        """A pose schedule: the factor on the six pose weights (the first six diagonal entries of Q / P: rotation error, then
        translation error) that knot i of trajectory b reads.  [B, N+1, 6]; [N+1, 6], every trajectory the same; [B, N+1] or
        [N+1], one factor for all six coordinates (a 2-D array of shape (N+1, 6) is read as [N+1, 6]).  Checked on the host:
        ValueError for another shape, a non-finite or a negative entry.  Returns [B, N+1, 6] float64 numpy, or None when
        omitted (no schedule)."""
        if pose_scale is None:
            return None
        a = _checked("pose_scale", pose_scale, (None,) * np.ndim(pose_scale), finite=True)
        n = self.N + 1
        if a.shape == (B, n, 6):
            pass
        elif a.shape == (n, 6):
            a = np.broadcast_to(a, (B, n, 6))
        elif a.shape == (B, n):
            a = np.broadcast_to(a[:, :, None], (B, n, 6))
        elif a.shape == (n,):
            a = np.broadcast_to(a[None, :, None], (B, n, 6))
        else:
            raise ValueError("pose_scale has shape %s, expected (%d, %d, 6), (%d, 6), (%d, %d) or (%d,)"
                             % (tuple(a.shape), B, n, n, B, n, n))
        if np.any(a < 0.0):
            raise ValueError("pose_scale must not be negative")
        return np.ascontiguousarray(a)

    def _own_weights(self, B):
        """The problem's own Q, P, R as per-trajectory diagonals (q [B, 12], p [B, 12], r [B, m]): what a pose schedule sits
        on when the caller gives no weights.  ValueError when one of them is not diagonal: the per-trajectory kernels read
        diagonals only."""
        out = []
        for name, a, n in (("Q", self.problem.Q, 12), ("P", self.problem.P, 12), ("R", self.problem.R, self.m)):
            a = np.asarray(a, dtype=np.float64).reshape(n, n)
            if np.any(a - np.diag(np.diag(a)) != 0.0):
                raise ValueError("a pose schedule sits on per-trajectory (diagonal) weights: the problem's %s is not diagonal" % name)
            out.append(np.ascontiguousarray(np.broadcast_to(np.diag(a), (B, n))))
        return tuple(out)

    def _check_xs_init(self, B, xs_init, mode):
        """xs_init = (xs_q [B, N+1, 4, 4], xs_xi [B, N+1, 6]) checked on the host; None when omitted."""
        if xs_init is None:
            return None
        if mode != "ms":
            raise ValueError("xs_init warm-starts the shooting states of multiple shooting: single shooting takes its states "
                             "from the initial rollout")
        if not isinstance(xs_init, (tuple, list)) or len(xs_init) != 2:
            raise ValueError("xs_init is a pair (xs_q [B, N+1, 4, 4], xs_xi [B, N+1, 6])")
        return _checked("xs_init[0]", xs_init[0], (B, self.N + 1, 4, 4)), _checked("xs_init[1]", xs_init[1], (B, self.N + 1, 6))

    def _stage(self, x_q, x_xi, us, refs=(None, None), weights=(None, None, None), xs_init=None, mode="ms", traj=False,
               pose_scale=None):
        """The one way a batch's inputs reach the device: x_q reshaped to [B, 16] gives B (traj=True: whole trajectories
        [B, N+1, 16], linearize_backward), then the per-trajectory references (q_ref, xi_ref), weights (Q, P, R), the pose
        schedule and xs_init are checked on the host, and everything moves to the device.  us = None: zeros (not for
        trajectories).  A schedule without weights sits on the problem's own (_own_weights); with no pose_scale the call
        takes the windows set_pose_schedule_windows staged for it, if any."""
        k = (self.N + 1,) if traj else ()
        x_q = self._dev(x_q, (-1,) + k + (16,))
        B = x_q.shape[0]
        refs = self._check_refs(B, *refs)
        wts = self._check_weights(B, *weights)
        sched = self._check_pose_scale(B, pose_scale)
        staged, self._sched_next = self._sched_next, None
        if sched is not None:
            sched = (self._dev(sched, sched.shape),)
        elif staged is not None:
            if staged[0].shape[0] != B:
                raise ValueError("set_pose_schedule_windows staged a schedule for %d trajectories, this call has %d"
                                 % (staged[0].shape[0], B))
            sched = staged
        if sched is not None and wts is None:
            wts = self._own_weights(B)
        xs = self._check_xs_init(B, xs_init, mode)
        x_xi = self._dev(x_xi, (B,) + k + (6,))
        if us is None and not traj:
            us = torch.zeros(B, self.N, self.m, dtype=torch.float64, device=self.device)
        pair = lambda p: None if p is None else (self._dev(p[0], (B, self.N + 1, 16)), self._dev(p[1], (B, self.N + 1, 6)))  # noqa: E731
        return _Batch(B, x_q, x_xi, self._dev(us, (B, self.N, self.m)), pair(refs),
                      None if wts is None else tuple(self._dev(a, a.shape) for a in wts), pair(xs), sched)

    def clear_per_trajectory(self):
        """Return the handle to the problem's shared reference and weights, without a pose schedule (tolg_set_pose_schedule /
        tolg_set_refs / tolg_set_weights with NULL).  The solve calls do this themselves when they are given no per-trajectory
        inputs; this is for callers that drove the C ABI on the handle directly."""
        self._sched_next = None
        self._detach("tolg_set_pose_schedule")
        self._detach("tolg_set_weights")
        self._detach("tolg_set_refs")
        self._wts_set = self._refs_set = False

    def _use_pt(self, B, refs, wts, sched=None):
        """Point the handle at this call's references (tolg_set_refs), weights (tolg_set_weights) and the pose schedule on
        them (_Batch.sched), device tensors of a _Batch, or back at the problem's shared ones for what is None: every call
        states its own, nothing carries over from an earlier call.  The weights are detached first (their schedule goes with
        them), so that references for a new B never meet weights set for an earlier one."""
        if self._wts_set:
            self._detach("tolg_set_weights")
            self._wts_set = False
        self._use_refs(B, refs)
        if wts is not None:
            self._call("tolg_set_weights", B, *map(_ptr, wts), *self._packed("_wts_buf", self.lib.tolg_weights_bytes))
            self._wts_set = True
        if sched is not None:
            self._set_pose_schedule(B, sched)

    def _set_pose_schedule(self, B, sched):
        """tolg_set_pose_schedule(_windows) of a _Batch.sched on the weights the handle holds for B."""
        dest = self._packed("_sched_buf", self.lib.tolg_pose_schedule_bytes)
        if len(sched) == 1:
            self._call("tolg_set_pose_schedule", B, _ptr(sched[0]), *dest)
        else:
            path, T, t0_d, t = sched
            self._call("tolg_set_pose_schedule_windows", B, _ptr(path), int(T), _ptr(t0_d), int(t), *dest)

    def _use_refs(self, B, refs):
        """Point the handle at the references refs = (q [B, N+1, 4, 4], xi [B, N+1, 6]) (tolg_set_refs), or back at the
        problem's shared one when refs is None."""
        if refs is not None:
            q, xi = self._dev(refs[0], (B, self.N + 1, 16)), self._dev(refs[1], (B, self.N + 1, 6))  # (staged: views)
            self._call("tolg_set_refs", B, _ptr(q), _ptr(xi), *self._packed("_refs_buf", self.lib.tolg_refs_bytes))
            self._refs_set = True
        elif self._refs_set:
            self._detach("tolg_set_refs")
            self._refs_set = False

    # ------------------------------------------------------------------------------------------
    def _alloc_result(self, B, K, histories=True):
        f64 = dict(dtype=torch.float64, device=self.device)
        nanf = lambda *shape: torch.full(shape, float("nan"), **f64) if histories else None  # noqa: E731
        return FitResult(
            xs_q=torch.empty(B, self.N + 1, 4, 4, **f64), xs_xi=torch.empty(B, self.N + 1, 6, **f64),
            us=torch.empty(B, self.N, self.m, **f64), J_hist=nanf(B, K), grad_hist=nanf(B, K + 1),
            defect_hist=nanf(B, K + 1), alpha_hist=nanf(B, K), mu_hist=nanf(B, K),
            iters=torch.zeros(B, dtype=torch.int32, device=self.device),
            status=torch.zeros(B, dtype=torch.int32, device=self.device),
            converged=torch.zeros(B, dtype=torch.int32, device=self.device))

    def solve_begin(self, x0_q, x0_xi, us_init=None, mode="ms", n_iterations=100, tol_grad_norm=1e-6,
                    tol_d_norm=1e-6, line_search=False, rollout="nonlinear", max_reg=1e10, histories=True,
                    out: Optional[FitResult] = None, schedule="auto", q_ref=None, xi_ref=None, Q=None, P=None,
                    R=None, xs_init=None, pose_scale=None) -> FitResult:
        """_initial_guess + first _linearization; leaves the batch resident in HBM.
        schedule: "auto" (rollout and re-linearisation fused in one launch where the mode allows it) or
        "split" (separate launches); launch structure only, same algorithm.
        q_ref [B, N+1, 4, 4], xi_ref [B, N+1, 6] (optional): trajectory b tracks its own reference in this solve
        (tolg_set_refs); omitted, the problem's shared reference.
        Q [B, 12, 12], P [B, 12, 12], R [B, m, m] (optional, all three or none, diagonal): trajectory b's cost weights in this
        solve (tolg_set_weights); omitted, the problem's shared weights.
        pose_scale (optional): a schedule on the pose weights, a factor per knot (_check_pose_scale: [B, N+1, 6], [N+1, 6],
        [B, N+1] or [N+1]; tolg_set_pose_schedule): knot i of trajectory b weights its pose error with pose_scale[b, i] times
        the first six diagonal entries of Q (of P where the knot reads P).  Pose weights only: twist weights and R stay
        constant along the horizon.  Without Q / P / R it sits on the problem's own weights, which must then be diagonal.
        xs_init (optional, multiple shooting only): (xs_q [B, N+1, 4, 4], xs_xi [B, N+1, 6]), a warm start of the shooting
        states (tolg_solve_begin_warm): knots 1..N of the initial guess in place of the reference; knot 0 is x0."""
        b = self._stage(x0_q, x0_xi, us_init, (q_ref, xi_ref), (Q, P, R), xs_init, mode, pose_scale=pose_scale)
        o = self._options(mode, n_iterations, line_search, rollout, tol_grad_norm, tol_d_norm, max_reg, schedule)
        return self._start(b, o, histories, out)

    def _options(self, mode, K, line_search, rollout, tol_grad_norm, tol_d_norm, max_reg, schedule="auto", check_every=0):
        return _capi.Options(_capi.MODE_MS if mode == "ms" else _capi.MODE_SS, int(K), int(bool(line_search)),
                             int(rollout == "linear"), float(tol_grad_norm), float(tol_d_norm),
                             float(max_reg if max_reg else 0.0),
                             {"auto": _capi.SCHED_AUTO, "split": _capi.SCHED_SPLIT}[schedule], int(check_every))

    def _start(self, b, o, histories=True, out=None):
        """solve_begin on a staged batch: the handle pointed at its references and weights, then its solve begun."""
        if out is None:
            out = self._alloc_result(b.B, o.max_iter, histories)
        self._use_pt(b.B, b.refs, b.wts, b.sched)
        self._hold(b)
        return self._begin(o, b.B, b.x_q, b.x_xi, b.us, b.xs, out)

    def _begin(self, o, B, x0_q, x0_xi, us_init, xs, out):
        """tolg_solve_begin, or tolg_solve_begin_warm when xs = (xs_q, xs_xi) is given (device tensors, checked)."""
        hist = (_ptr(out.J_hist), _ptr(out.grad_hist), _ptr(out.defect_hist), _ptr(out.alpha_hist), _ptr(out.mu_hist))
        if xs is None:
            self._call("tolg_solve_begin", C.byref(o), B, _ptr(x0_q), _ptr(x0_xi), _ptr(us_init), *hist)
        else:
            self._call("tolg_solve_begin_warm", C.byref(o), B, _ptr(x0_q), _ptr(x0_xi), _ptr(xs[0]), _ptr(xs[1]), _ptr(us_init),
                       *hist)
        self._inflight = (out, self._inflight[1])
        return out

    def solve_iterate(self, n_iter):
        """n_iter passes of the iteration body (backward sweep, rollout, re-linearisation)."""
        self._call("tolg_solve_iterate", int(n_iter))

    def solve_iterate_until(self, n_iter, check_every) -> int:
        """Up to n_iter iterations in slices of check_every, stopping once no trajectory is iterating any more
        (tolg_solve_iterate_until: the read-back of one slice overlaps the next).  Returns the iterations queued."""
        n = C.c_int32(0)
        self._call("tolg_solve_iterate_until", int(n_iter), int(check_every), C.byref(n))
        return int(n.value)

    def active_count(self) -> int:
        """Trajectories of the solve in flight that are still being iterated (one small kernel + a host read)."""
        if getattr(self, "_active_buf", None) is None:
            self._active_buf = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._call("tolg_solve_active_count", _ptr(self._active_buf))
        return int(self._active_buf.item())

    def _export(self, fn):
        out = self._inflight[0]
        self._call(fn, _ptr(out.xs_q), _ptr(out.xs_xi), _ptr(out.us), _ptr(out.iters), _ptr(out.status), _ptr(out.converged),
                   batch=out.xs_q.shape[0])
        return out

    def solve_peek(self) -> FitResult:
        """Export the trajectories in flight (xs, us, iters, status) without ending the solve."""
        return self._export("tolg_solve_peek")

    def solve_end(self) -> FitResult:
        return self._export("tolg_solve_end")

    def fit_batch(self, x0_q, x0_xi, us_init=None, mode="ms", n_iterations=100, tol_grad_norm=1e-6,
                  tol_d_norm=1e-6, line_search=False, rollout="nonlinear", max_reg=1e10,
                  histories=True, out: Optional[FitResult] = None, schedule="auto", check_every=16, q_ref=None,
                  xi_ref=None, Q=None, P=None, R=None, xs_init=None, pose_scale=None) -> FitResult:
        """B independent fits (the reference's joblib fan-out, visualization/perturb_all_compute.py:240).
        Inputs may be numpy arrays or tensors already on the device; outputs are device tensors.
        The iterations are issued in slices of `check_every`; behind each slice the number of trajectories still
        iterating is read back (overlapped with the next slice) and the loop stops when it reaches zero (the early
        exit of traopt_controller.py:2528-2532 for the whole batch).  check_every=0, or tolerances of zero, issue
        all n_iterations without a host read.  `iterations_issued` keeps how many were queued.
        q_ref [B, N+1, 4, 4], xi_ref [B, N+1, 6] (optional, numpy or torch): a reference per trajectory for this fit.
        Q [B, 12, 12], P [B, 12, 12], R [B, m, m] (optional, all three or none, diagonal): cost weights per trajectory.
        pose_scale (optional): a per-knot schedule on the pose weights, as for solve_begin.
        xs_init (optional, mode="ms"): warm-start shooting states, as for solve_begin."""
        b = self._stage(x0_q, x0_xi, us_init, (q_ref, xi_ref), (Q, P, R), xs_init, mode, pose_scale=pose_scale)
        o = self._options(mode, n_iterations, line_search, rollout, tol_grad_norm, tol_d_norm, max_reg, schedule)
        return self._fit(b, o, check_every, histories, out)

    def _fit(self, b, o, check_every, histories=True, out=None):
        self._start(b, o, histories, out)
        self.iterations_issued = self.solve_iterate_until(o.max_iter, int(check_every or 0))
        return self.solve_end()

    def solve_batch_one_call(self, x0_q, x0_xi, us_init=None, mode="ms", n_iterations=100, tol_grad_norm=1e-6,
                             tol_d_norm=1e-6, line_search=False, rollout="nonlinear", max_reg=1e10, schedule="auto",
                             check_every=0, q_ref=None, xi_ref=None, Q=None, P=None, R=None, pose_scale=None) -> FitResult:
        """The same fit through the single entry point tolg_solve_batch (what a C / C++ caller binds): begin,
        iterations (tolg_options.check_every: 0 = all of them, never synchronising), end in one call.
        q_ref / xi_ref, Q / P / R, pose_scale: as for fit_batch."""
        b = self._stage(x0_q, x0_xi, us_init, (q_ref, xi_ref), (Q, P, R), pose_scale=pose_scale)
        K = int(n_iterations)
        out = self._alloc_result(b.B, K, True)
        o = self._options(mode, K, line_search, rollout, tol_grad_norm, tol_d_norm, max_reg, schedule, check_every)
        self._use_pt(b.B, b.refs, b.wts, b.sched)
        self._hold(b)
        self._call("tolg_solve_batch", C.byref(o), b.B, _ptr(b.x_q), _ptr(b.x_xi), _ptr(b.us), _ptr(out.xs_q), _ptr(out.xs_xi),
                   _ptr(out.us), _ptr(out.J_hist), _ptr(out.grad_hist), _ptr(out.defect_hist), _ptr(out.alpha_hist),
                   _ptr(out.mu_hist), _ptr(out.iters), _ptr(out.status), _ptr(out.converged), batch=b.B)
        torch.cuda.current_stream(self.device).synchronize()  # the call returns with its results in place
        return out

    # ------------------------------------------------------------------------------------------
    def set_al(self, lb=None, ub=None, lam=None, imu=None):
        """Attach (or detach with lb=None) the augmented-Lagrangian box input constraint terms
        (ALConstrainedCost + InputConstraint).  lam, imu: device tensors [B, N, 2m].  lb, ub [m]: one box for every
        trajectory and knot (tolg_set_al); [B, m]: a box per trajectory, or [B, N, m]: per knot as well (check_input_box;
        tolg_set_al_box, which reads the bounds in place beside the multipliers: every batch call must then be for this B;
        not for the SO3 family and the pendulum).  Each attach replaces the one before, whatever its shape."""
        if lb is None:
            self._al = None
            self._detach("tolg_set_al")
        elif np.ndim(lb) <= 1:
            lb = self._dev(lb, (self.m,)); ub = self._dev(ub, (self.m,))
            self._al = (lb, ub, lam, imu)  # the handle reads them in every solve until they are detached
            self._call("tolg_set_al", _ptr(lb), _ptr(ub), _ptr(lam), _ptr(imu), stream=False)
        else:
            B = self._box_multipliers(lam, imu)
            lo, hi = check_input_box(lb, ub, B, self.N, self.m)
            lo, hi = self._dev(lo, lo.shape), self._dev(hi, hi.shape)
            self._call("tolg_set_al_box", B, _capi.BOX_PER_KNOT if lo.dim() == 3 else _capi.BOX_PER_TRAJECTORY, _ptr(lo), _ptr(hi),
                       _ptr(lam), _ptr(imu), stream=False)
            self._al = (lo, hi, lam, imu)

    def _box_multipliers(self, lam, imu):
        """The box's multipliers lam, imu [B, N, 2m] checked where their batch decides how the bounds are read (contiguous
        float64 on the device); returns B."""
        if self.problem.kind in ("so3", "pendulum3d"):
            raise ValueError("an input box per trajectory or per knot is not offered for the %s model: it takes lb, ub [m]"
                             % self.problem.kind)
        for name, t in (("lam", lam), ("imu", imu)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64 tensor on %s" % (name, self.device))
            _checked(name, t, (lam.shape[0] if lam.dim() else None, self.N, 2 * self.m))
        B = int(lam.shape[0])
        if not 1 <= B <= self.max_batch:
            raise ValueError("an input box for B = %d trajectories, expected 1..%d" % (B, self.max_batch))
        return B

    def set_al_box_windows(self, path_lb, path_ub, t, t0=None, lam=None, imu=None):
        """Attach the input boxes of step t, gathered on the device from world-time paths (tolg_set_al_box_windows): path_lb,
        path_ub [B, T+1, m], the bounds of trajectory b at world knot s (finite, lb <= ub); knot i of the window takes world
        knot min(t0[b] + t + i, T), set_ref_windows' rule (t0 an int array [B], None: 0).  The handle is then as after set_al
        with the gathered [B, N, m] bounds; lam, imu [B, N, 2m] as there.  path_lb = None detaches."""
        if path_lb is None:
            return self.set_al(None)
        if int(t) < 0:
            raise ValueError("t must be non-negative")
        B = self._box_multipliers(lam, imu)
        lo, hi = self._box_paths(B, path_lb, path_ub)
        t0_d = self._check_t0(B, t0)
        self._hold((lo, hi, t0_d))
        self._set_box_windows(B, lo, hi, t0_d, int(t), lam, imu)

    def _box_paths(self, B, path_lb, path_ub):
        """World-time box paths [B, T+1, m] checked on the host under check_input_box's rule (T >= 1 in place of the horizon)
        and moved to the device."""
        n = np.shape(path_lb)[1] if np.ndim(path_lb) == 3 else 0
        if n < 2:
            raise ValueError("lb_path has shape %s, expected (%d, T+1 >= 2, %d)" % (tuple(np.shape(path_lb)), B, self.m))
        lo, hi = check_input_box(path_lb, path_ub, B, n, self.m)
        return self._dev(lo, lo.shape), self._dev(hi, hi.shape)

    def _set_box_windows(self, B, d_lb, d_ub, t0_d, t, lam, imu):
        f64 = dict(dtype=torch.float64, device=self.device)
        win = self._box_win
        if win is None or win[0].shape[0] != B:  # the caller-owned windows the handle reads in place until the next attach
            win = self._box_win = (torch.empty(B, self.N, self.m, **f64), torch.empty(B, self.N, self.m, **f64))
        self._call("tolg_set_al_box_windows", B, _ptr(d_lb), _ptr(d_ub), int(d_lb.shape[1] - 1), _ptr(t0_d), int(t), _ptr(win[0]),
                   _ptr(win[1]), _ptr(lam), _ptr(imu))
        self._al = (win[0], win[1], lam, imu, d_lb, d_ub)

    def _check_obstacles(self, B, obstacles, kinds=None):
        """Keep-out spheres [K, 4] (every trajectory the same), [B, K, 4], or per knot [B, N+1, K, 4], rows (cx, cy, cz, r),
        checked on the host: ValueError before anything reaches the device for a model without translation, a wrong shape (the
        per-knot form must have N + 1 knots), K outside 1..MAX_OBSTACLES, a non-finite value or a radius that is not positive
        at any knot.  B = None takes B from a [B, K, 4] or [B, N+1, K, 4] array.  Returns (B, [B, K, 4] or [B, N+1, K, 4]
        float64 numpy).  kinds: the slots' kinds (check_kinds), which decide how the four fields are read and checked
        (check_kind_geometry)."""
        if self.problem.kind in ("so3", "pendulum3d"):
            raise ValueError("keep-out spheres constrain the translation: the %s model has none" % self.problem.kind)
        a = obstacles.detach().cpu().numpy() if isinstance(obstacles, torch.Tensor) else obstacles
        a = np.asarray(a, dtype=np.float64)
        if a.ndim not in (2, 3, 4):
            raise ValueError("obstacles has shape %s, expected (K, 4), (B, K, 4) or (B, N+1, K, 4)" % (a.shape,))
        a = _checked("obstacles", a, (None,) * a.ndim, finite=True)
        if a.ndim == 2:
            if B is None:
                raise ValueError("obstacles [K, 4] need the batch: give lam / imu [B, N+1, K] or obstacles [B, K, 4]")
            a = np.broadcast_to(a, (B,) + a.shape)
        B = a.shape[0] if B is None else B
        a = _checked("obstacles", a, (B, None, 4) if a.ndim == 3 else (B, self.N + 1, None, 4))
        if not 1 <= a.shape[-2] <= _capi.MAX_OBSTACLES:
            raise ValueError("obstacles: K = %d spheres per trajectory, expected 1..%d" % (a.shape[-2], _capi.MAX_OBSTACLES))
        check_kind_geometry("obstacles", a, check_kinds(kinds, a.shape[-2]))
        return B, np.ascontiguousarray(a)

    def _set_kinds(self, K, kinds):
        """Behind an attach of K slots: the handle keeps its kinds over a re-attach with the same K and resets them otherwise
        (tolg_set_al_obstacle_kinds), so the call is made only where what it holds is not `kinds`."""
        held = self._obs_kinds if len(self._obs_kinds) == K else (0,) * K
        if kinds != held:
            arr = (C.c_int32 * K)(*kinds)
            self._call("tolg_set_al_obstacle_kinds", K, arr if any(kinds) else None)
        self._obs_kinds = kinds

    def set_al_obstacles(self, obstacles=None, lam=None, imu=None, kinds=None):
        """Attach (or detach with obstacles=None) keep-out spheres: the augmented-Lagrangian terms of g_k = r_k^2 - |t - c_k|^2
        <= 0 at every knot, terminal included (tolg_set_al_obstacles).  obstacles [K, 4] (broadcast) or [B, K, 4] rows (cx, cy,
        cz, r), or [B, N+1, K, 4]: spheres that move, the geometry of every knot (tolg_set_al_obstacles_moving; its packed
        buffer, N + 1 times the static one, is allocated for the B and K asked for); lam, imu [B, N+1, K]: the multipliers and the diagonal of I_mu (device tensors the handle reads in every solve
        until they are detached; None: zeros).  Every batch call must then be for this B.
        kinds: a length-K sequence of ints or of "sphere" | "keep_in" | "half_space" | "column" (OBSTACLE_KINDS), the kind of
        slot k in every trajectory and at every knot; None: keep-out spheres.  The fields of a slot are then read per kind:
        (cx, cy, cz, r) with g = |d|^2 - r^2 for a keep-in sphere, (nx, ny, nz, o) with |n| = 1 and g = n.t - o for a
        half-space, (cx, cy, -, r) with g = r^2 - (dx^2 + dy^2) for a vertical column."""
        if obstacles is None:
            self._obs, self._obs_kinds = None, ()
            self._detach("tolg_set_al_obstacles")
            return
        Bl = None if lam is None else int(lam.shape[0])
        B, a = self._check_obstacles(Bl, obstacles, kinds)
        kinds = check_kinds(kinds, a.shape[-2])
        K, moving = a.shape[-2], a.ndim == 4
        lam, imu = self._obs_multipliers(B, K, lam, imu)
        dest = (self._packed("_obs_mov_buf", self.lib.tolg_obstacles_moving_bytes, K, B=B) if moving else
                self._packed("_obs_buf", self.lib.tolg_obstacles_bytes, _capi.MAX_OBSTACLES))
        d = self._dev(a, a.shape)
        self._obs = (d, lam, imu)  # the handle reads the multipliers in every solve until they are detached
        self._call("tolg_set_al_obstacles" + ("_moving" if moving else ""), B, K, _ptr(d), _ptr(lam), _ptr(imu), *dest)
        self._set_kinds(K, kinds)

    def _obs_multipliers(self, B, K, lam, imu):
        """The spheres' multipliers lam, imu [B, N+1, K] checked (contiguous float64 on the device; None: zeros), and B."""
        f64 = dict(dtype=torch.float64, device=self.device)
        if lam is None:
            lam = torch.zeros(B, self.N + 1, K, **f64)
        if imu is None:
            imu = torch.zeros(B, self.N + 1, K, **f64)
        for name, t in (("lam", lam), ("imu", imu)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64 tensor on %s" % (name, self.device))
            _checked(name, t, (B, self.N + 1, K))
        if not 1 <= B <= self.max_batch:
            raise ValueError("obstacles for B = %d trajectories, expected 1..%d" % (B, self.max_batch))
        return lam, imu

    def _check_obstacle_paths(self, B, path_obs, kinds=None):
        """World-time sphere paths [B, T+1, K, 4], rows (cx, cy, cz, r), checked under _check_obstacles' rules (T >= 1 in place of
        the horizon).  The paths are large (116 MB at 4096 x 220, K = 4): a tensor that is on the solver's device already is
        checked there -- two reductions and one flag read back -- and never copied through the host; anything else is checked
        on the host.  B = None takes it from the array.  Returns (B, the paths: that device tensor, or a float64 numpy array)."""
        if self.problem.kind in ("so3", "pendulum3d"):
            raise ValueError("keep-out spheres constrain the translation: the %s model has none" % self.problem.kind)
        on_device = isinstance(path_obs, torch.Tensor) and path_obs.device == self.device
        a = _checked("obstacle_paths", path_obs, (B, None, None, 4), finite=not on_device)
        if a.shape[1] < 2:
            raise ValueError("obstacle_paths has %d knots, expected T+1 >= 2" % a.shape[1])
        if not 1 <= a.shape[2] <= _capi.MAX_OBSTACLES:
            raise ValueError("obstacle_paths: K = %d spheres per trajectory, expected 1..%d" % (a.shape[2], _capi.MAX_OBSTACLES))
        kinds = check_kinds(kinds, a.shape[2])
        if on_device and not any(kinds):
            v = a.detach()
            finite, positive = (bool(f) for f in torch.stack([torch.isfinite(v).all(), (v[..., 3] > 0.0).all()]).tolist())
        elif on_device:
            finite, positive = bool(torch.isfinite(a.detach()).all()), True
        else:
            finite, positive = True, not (np.any(a[..., 3] <= 0.0) and not any(kinds))  # (_checked has refused a non-finite value)
        if not finite:
            raise ValueError("obstacle_paths must be finite")
        if not positive:
            raise ValueError("obstacle_paths: every radius must be positive")
        if any(kinds):
            check_kind_geometry("obstacle_paths", a.detach() if on_device else a, kinds)
        return a.shape[0], a if on_device else np.ascontiguousarray(a)

    def _set_obstacle_windows(self, B, d_paths, t0_d, t, lam, imu, kinds=None):
        K, T = d_paths.shape[2], d_paths.shape[1] - 1
        self._obs = (d_paths, lam, imu)
        self._call("tolg_set_al_obstacle_windows", B, K, _ptr(d_paths), int(T), _ptr(t0_d), int(t), _ptr(lam), _ptr(imu),
                   *self._packed("_obs_mov_buf", self.lib.tolg_obstacles_moving_bytes, K, B=B))
        self._set_kinds(K, check_kinds(kinds, K))

    def set_al_obstacle_windows(self, path_obs, t, t0=None, lam=None, imu=None, kinds=None):
        """Attach the moving keep-out spheres of step t, gathered on the device from world-time paths
        (tolg_set_al_obstacle_windows): path_obs [B, T+1, K, 4] rows (cx, cy, cz, r) of trajectory b's spheres at world knot s;
        knot i of the window takes world knot min(t0[b] + t + i, T), set_ref_windows' rule (t0 an int array [B], None: 0).  The
        handle is then as after set_al_obstacles with the gathered [B, N+1, K, 4] field; lam, imu [B, N+1, K] and kinds as
        there.  path_obs = None detaches."""
        if path_obs is None:
            return self.set_al_obstacles(None)
        if int(t) < 0:
            raise ValueError("t must be non-negative")
        B, a = self._check_obstacle_paths(None if lam is None else int(lam.shape[0]), path_obs, kinds)
        lam, imu = self._obs_multipliers(B, a.shape[2], lam, imu)
        t0_d = self._check_t0(B, t0)
        d = self._dev(a, a.shape)
        self._hold((d, t0_d))
        self._set_obstacle_windows(B, d, t0_d, int(t), lam, imu, kinds)

    def _check_pose_constraints(self, B, slots, kinds):
        """Pose slots [K, 4] (every trajectory the same), [B, K, 4], or per knot [B, N+1, K, 4], fields per kind (check_pose_kinds,
        check_pose_geometry), checked on the host: ValueError before anything reaches the device for a model of the SO3 family,
        a wrong shape, K outside 1..MAX_POSE_CONSTRAINTS, a non-finite value, an axis that is not unit or a cosine outside
        (-1, 1).  B = None takes B from a [B, ...] array.  Returns (B, [B, K, 4] or [B, N+1, K, 4] float64 numpy, kinds)."""
        if self.problem.kind in ("so3", "pendulum3d"):
            raise ValueError("pose constraints are not offered for the %s model" % self.problem.kind)
        a = slots.detach().cpu().numpy() if isinstance(slots, torch.Tensor) else slots
        a = np.asarray(a, dtype=np.float64)
        if a.ndim not in (2, 3, 4):
            raise ValueError("pose constraints have shape %s, expected (K, 4), (B, K, 4) or (B, N+1, K, 4)" % (a.shape,))
        a = _checked("pose_constraints", a, (None,) * a.ndim, finite=True)
        if a.ndim == 2:
            if B is None:
                raise ValueError("pose constraints [K, 4] need the batch: give lam / imu [B, N+1, K] or slots [B, K, 4]")
            a = np.broadcast_to(a, (B,) + a.shape)
        B = a.shape[0] if B is None else B
        a = _checked("pose_constraints", a, (B, None, 4) if a.ndim == 3 else (B, self.N + 1, None, 4))
        if not 1 <= a.shape[-2] <= _capi.MAX_POSE_CONSTRAINTS:
            raise ValueError("pose constraints: K = %d slots per trajectory, expected 1..%d" % (a.shape[-2], _capi.MAX_POSE_CONSTRAINTS))
        if not 1 <= B <= self.max_batch:
            raise ValueError("pose constraints for B = %d trajectories, expected 1..%d" % (B, self.max_batch))
        kinds = check_pose_kinds(kinds, a.shape[-2])
        check_pose_geometry("pose_constraints", a, kinds)
        return B, np.ascontiguousarray(a), kinds

    def set_al_pose_constraints(self, slots=None, kinds=None, lam=None, imu=None):
        """Attach (or detach with slots=None) pose constraints, the second slot family (tolg_set_al_pose_constraints): the
        augmented-Lagrangian terms of g_k(R, t) <= 0 at every knot, terminal included, beside whatever set_al /
        set_al_obstacles attached.  slots [K, 4] (broadcast), [B, K, 4], or per knot [B, N+1, K, 4]; kinds a length-K sequence
        of ints or of "tilt_cone" | "view_cone" (POSE_CONSTRAINT_KINDS), the kind of slot k in every trajectory and at every
        knot.  A tilt cone has fields (nx, ny, nz, c): never tilt the body axis e3 more than acos(c) from the unit world axis
        n, g = c - n^T R e3.  A view cone has fields (px, py, pz, c): keep the world target p within acos(c) of the forward
        axis e1, g = c |b| - e1^T b with b = R^T (p - t).  lam, imu [B, N+1, K]: the multipliers and the diagonal of I_mu
        (device tensors the handle reads in every solve until they are detached; None: zeros).  Every batch call must then
        be for this B; mpc() and plan_fleet take pose slots of their own (pose_constraints=) and refuse a family the caller
        attached here."""
        if slots is None:
            self._pose = None
            self._detach("tolg_set_al_pose_constraints")
            return
        Bl = None if lam is None else int(lam.shape[0])
        B, a, kinds = self._check_pose_constraints(Bl, slots, kinds)
        K, per_knot = a.shape[-2], a.ndim == 4
        lam, imu = self._obs_multipliers(B, K, lam, imu)
        fn = self.lib.tolg_pose_constraints_bytes
        dest = self._packed("_pose_knot_buf", fn, K, 1, B=B) if per_knot else self._packed("_pose_buf", fn, _capi.MAX_POSE_CONSTRAINTS, 0)
        d = self._dev(a, a.shape)
        self._call("tolg_set_al_pose_constraints", B, K, (C.c_int32 * K)(*kinds), _ptr(d), int(per_knot), _ptr(lam), _ptr(imu), *dest)
        self._pose = (d, lam, imu, kinds)  # the handle reads the multipliers in every solve until they are detached

    def _check_pose_paths(self, B, path_slots, kinds):
        """World-time pose slots [B, T+1, K, 4] checked on the host under _check_pose_constraints' rules (T >= 1 in place of the
        horizon), the geometry over the whole path.  As _check_obstacle_paths, a tensor that is on the solver's device already is
        checked there (check_pose_geometry's reductions) and never copied through the host.  B = None takes it from the array.
        Returns (B, the paths: that device tensor, or a float64 numpy array, kinds)."""
        if self.problem.kind in ("so3", "pendulum3d"):
            raise ValueError("pose constraints are not offered for the %s model" % self.problem.kind)
        on_device = isinstance(path_slots, torch.Tensor) and path_slots.device == self.device
        a = _checked("pose_paths", path_slots, (B, None, None, 4), finite=not on_device)
        if a.shape[1] < 2:
            raise ValueError("pose_paths has %d knots, expected T+1 >= 2" % a.shape[1])
        if not 1 <= a.shape[2] <= _capi.MAX_POSE_CONSTRAINTS:
            raise ValueError("pose_paths: K = %d slots per trajectory, expected 1..%d" % (a.shape[2], _capi.MAX_POSE_CONSTRAINTS))
        if not 1 <= a.shape[0] <= self.max_batch:
            raise ValueError("pose_paths for B = %d trajectories, expected 1..%d" % (a.shape[0], self.max_batch))
        kinds = check_pose_kinds(kinds, a.shape[2])
        check_pose_geometry("pose_paths", a.detach() if on_device else a, kinds)
        return a.shape[0], a if on_device else np.ascontiguousarray(a), kinds

    def _set_pose_windows(self, B, d_paths, t0_d, t, lam, imu, kinds):
        K, T = d_paths.shape[2], d_paths.shape[1] - 1
        self._call("tolg_set_al_pose_constraint_windows", B, K, (C.c_int32 * K)(*kinds), _ptr(d_paths), int(T), _ptr(t0_d), int(t),
                   _ptr(lam), _ptr(imu), *self._packed("_pose_knot_buf", self.lib.tolg_pose_constraints_bytes, K, 1, B=B))
        self._pose = (d_paths, lam, imu, kinds)

    def set_al_pose_constraint_windows(self, path_slots, t, t0=None, kinds=None, lam=None, imu=None):
        """Attach the pose slots of step t, gathered on the device from world-time paths (tolg_set_al_pose_constraint_windows):
        path_slots [B, T+1, K, 4], the fields of trajectory b's slots at world knot s (a view target that moves in world time);
        knot i of the window takes world knot min(t0[b] + t + i, T), set_ref_windows' rule (t0 an int array [B], None: 0).  The
        handle is then as after set_al_pose_constraints with the gathered [B, N+1, K, 4] slots; kinds, lam, imu [B, N+1, K] as
        there, the geometry checked over the whole path (check_pose_geometry).  path_slots = None detaches."""
        if path_slots is None:
            return self.set_al_pose_constraints(None)
        if int(t) < 0:
            raise ValueError("t must be non-negative")
        B, a, kinds = self._check_pose_paths(None if lam is None else int(lam.shape[0]), path_slots, kinds)
        lam, imu = self._obs_multipliers(B, a.shape[2], lam, imu)
        t0_d = self._check_t0(B, t0)
        d = self._dev(a, a.shape)
        self._hold((d, t0_d))
        self._set_pose_windows(B, d, t0_d, int(t), lam, imu, kinds)

    def al_mpc_step(self, xs_q, us, mu, mu_scale=10.0, mu_max=1e8, tol_constr=1e-2, shift=True):
        """The outer augmented-Lagrangian update of one MPC step over everything attached (tolg_al_mpc_step; with a pose family
        attached through this object tolg_al_mpc_step_pose): the multipliers
        of set_al / set_al_obstacles / set_al_pose_constraints follow lambda <- max(0, lambda + I_mu g) on the controls us
        [B, N, m] and the poses of xs_q [B, N+1, 4, 4] (device tensors; either may be None where nothing attached reads it: the
        spheres read the positions, the pose slots the whole pose), mu [B] (a float64 device tensor, updated in place) grows
        by mu_scale up to mu_max where the largest g reaches tol_constr, and with shift every multiplier set then moves one
        knot towards the start, the last knot held.  Nothing is sticky: a satisfied problem's
        multipliers still relax.  The held policy is left alone.  Returns max_violation [B]."""
        if not isinstance(mu, torch.Tensor) or mu.dtype != torch.float64 or mu.device != self.device or mu.dim() != 1 \
                or not mu.is_contiguous():
            raise ValueError("mu must be a contiguous float64 tensor of shape (B,) on %s" % self.device)
        B = int(mu.shape[0])
        xs_q = None if xs_q is None else self._dev(xs_q, (B, self.N + 1, 16))
        us = None if us is None else self._dev(us, (B, self.N, self.m))
        maxviol = torch.empty(B, dtype=torch.float64, device=self.device)
        self._hold((xs_q, us))
        self._al_step(B, xs_q, us, mu, mu_scale, mu_max, tol_constr, maxviol, shift)
        return maxviol

    def _al_step(self, B, xs_q, us, mu, mu_scale, mu_max, tol_constr, maxviol, shift):
        # (tolg_al_mpc_step keeps refusing a pose family: the step that takes it as a third row set is a call of its own)
        self._call("tolg_al_mpc_step_pose" if self._pose is not None else "tolg_al_mpc_step", B, _ptr(xs_q), _ptr(us), _ptr(mu), float(mu_scale), float(mu_max), float(tol_constr),
                   _ptr(maxviol), int(bool(shift)))

    def al_fit_batch(self, x0_q, x0_xi, us_init, lb=None, ub=None, n_al_iters=100, n_ilqr_iters=200, tol_grad_norm=1e-6,
                     tol_d_norm=1e-6, tol_constr=1e-2, mu0=1e-2, mu_scale=10.0, mu_max=1e8, line_search=False,
                     on_outer=None, q_ref=None, xi_ref=None, Q=None, P=None, R=None, obstacles=None, obstacle_kinds=None,
                     pose_scale=None, pose_constraints=None, pose_kinds=None):
        """AL_iLQR_Tracking_SE3_MS.fit (reference traoptlibrary/traopt_controller.py:3218-3267) for B
        independent problems: every outer iteration re-solves from (x0, us_init) -- no warm start, as in
        the reference -- then updates multipliers on the device.  Returns (FitResult, info dict).
        q_ref / xi_ref: a reference per trajectory, Q / P / R: weights per trajectory, pose_scale: a per-knot schedule on the
        pose weights, as for fit_batch.
        Constraints: the input box lb <= u <= ub (lb, ub [m], or a box per trajectory [B, m], or per trajectory and knot
        [B, N, m]: check_input_box, set_al), keep-out spheres obstacles ([K, 4], [B, K, 4] or per knot [B, N+1, K, 4],
        set_al_obstacles; obstacle_kinds: its kinds=, a kind per slot -- keep-in sphere, half-space, column), or both
        (one mu per problem, joint convergence: tolg_al_update_state).  With spheres the info dict also holds lmbd_obs and
        Imu_obs [B, N+1, K]; max_violation covers every constraint.
        pose_constraints / pose_kinds: pose slots and their kinds (set_al_pose_constraints: tilt cones, view cones), alone or
        beside the others under the same mu and the same convergence; the info dict then holds lmbd_pose and Imu_pose
        [B, N+1, K]."""
        if (lb is None) != (ub is None):
            raise ValueError("the input box needs both lb and ub")
        if lb is None and obstacles is None and pose_constraints is None:
            raise ValueError("al_fit_batch needs a constraint: lb / ub, obstacles, pose_constraints, or several")
        b = self._stage(x0_q, x0_xi, us_init, (q_ref, xi_ref), (Q, P, R), pose_scale=pose_scale)
        B = b.B
        if obstacles is None and obstacle_kinds is not None:
            raise ValueError("obstacle_kinds describe obstacles: none were given")
        obs = None if obstacles is None else self._check_obstacles(B, obstacles, obstacle_kinds)[1]
        if pose_constraints is None and pose_kinds is not None:
            raise ValueError("pose_kinds describe pose_constraints: none were given")
        pose = None if pose_constraints is None else self._check_pose_constraints(B, pose_constraints, pose_kinds)[1:]
        o = self._options("ms", n_ilqr_iters, line_search, "nonlinear", tol_grad_norm, tol_d_norm, 1e10)
        f64 = dict(dtype=torch.float64, device=self.device)
        box = lb is not None
        lam = torch.zeros(B, self.N, 2 * self.m, **f64) if box else None
        imu = torch.full((B, self.N, 2 * self.m), float(mu0), **f64) if box else None
        mu = torch.full((B,), float(mu0), **f64)
        maxviol = torch.zeros(B, **f64)
        alconv = torch.zeros(B, dtype=torch.int32, device=self.device)
        lam_o = imu_o = None
        if box:
            lb_h, ub_h = check_input_box(lb, ub, B, self.N, self.m)
            self.set_al(lb_h, ub_h, lam, imu)  # (uploads them, once)
            lb_d, ub_d = self._al[0], self._al[1]
        shared_box = box and lb_d.dim() == 1  # tolg_al_update takes a [m] box of its own; the other forms are the handle's
        if obs is not None:
            lam_o = torch.zeros(B, self.N + 1, obs.shape[-2], **f64)
            imu_o = torch.full((B, self.N + 1, obs.shape[-2]), float(mu0), **f64)
            try:
                self.set_al_obstacles(obs, lam_o, imu_o, obstacle_kinds)
            except Exception:
                if box:
                    self.set_al(None)
                raise
        lam_p = imu_p = None
        if pose is not None:
            lam_p = torch.zeros(B, self.N + 1, pose[0].shape[-2], **f64)
            imu_p = torch.full((B, self.N + 1, pose[0].shape[-2]), float(mu0), **f64)
            try:
                self.set_al_pose_constraints(pose[0], pose[1], lam_p, imu_p)
            except Exception:
                if box:
                    self.set_al(None)
                if obs is not None:
                    self.set_al_obstacles(None)
                raise
        outer = 0
        res = None
        final = None
        try:
            for outer in range(int(n_al_iters)):
                res = self._fit(b, o, 16)
                if final is None:
                    final = res
                else:  # problems that had already converged keep the result of their converging solve
                    keep = alconv.bool()
                    for name in ("xs_q", "xs_xi", "us", "J_hist", "grad_hist", "defect_hist", "alpha_hist",
                                 "mu_hist", "iters", "status", "converged"):
                        new, old = getattr(res, name), getattr(final, name)
                        if new is not None:
                            new[keep] = old[keep]
                    final = res
                if on_outer is not None:  # before the multiplier update, like on_iteration_al (:3253-3259)
                    on_outer(outer, final, lam, imu, mu)
                if obs is None and pose is None and shared_box:
                    self._call("tolg_al_update", B, _ptr(final.us), _ptr(lb_d), _ptr(ub_d), _ptr(lam), _ptr(imu), _ptr(mu),
                               float(mu_scale), float(mu_max), float(tol_constr), _ptr(maxviol), _ptr(alconv))
                else:  # every attached constraint, one mu per problem
                    self._call("tolg_al_update_state", B, _ptr(final.xs_q), _ptr(final.us), _ptr(mu), float(mu_scale),
                               float(mu_max), float(tol_constr), _ptr(maxviol), _ptr(alconv))
                if bool(alconv.all().item()):
                    break
        finally:
            if box:
                self.set_al(None)
            if obs is not None:
                self.set_al_obstacles(None)
            if pose is not None:
                self.set_al_pose_constraints(None)
        info = dict(lmbd=lam, Imu=imu, mu=mu, max_violation=maxviol, al_converged=alconv, outer_iterations=outer + 1)
        if obs is not None:
            info.update(lmbd_obs=lam_o, Imu_obs=imu_o)
        if pose is not None:
            info.update(lmbd_pose=lam_p, Imu_pose=imu_p)
        return final, info

    def plan_fleet(self, x0_q, x0_xi, us_init, q_ref, xi_ref, fleet, separation, obstacles=None, lb=None, ub=None,
                   obstacle_kinds=None, pose_scale=None, pose_constraints=None, pose_kinds=None, **al_kw):
        """Prioritised planning for F = B / fleet independent fleets in one batch: trajectory b is member p = b % fleet of
        fleet b // fleet.  Round p = 0 .. fleet-1 solves the F members p, each on its own reference (q_ref [B, N+1, 4, 4],
        xi_ref [B, N+1, 6]), keeping out of the caller's static `obstacles` ([K0, 4] or [B, K0, 4]) and of p moving spheres of
        radius `separation` centred on the positions of members 0..p-1 of its fleet as their rounds left them
        (al_fit_batch with a per-knot field; lb / ub -- [m], or in batch order [B, m] / [B, N, m], every round takes
        its members' rows -- and al_kw -- n_al_iters, n_ilqr_iters, tol_constr, mu0, ..., Q / P / R
        [B, ...] -- go to it).  Round 0 with neither obstacles nor a box is a plain fit_batch with al_fit_batch's inner options.
        The constraint holds at the knots, not between them: two members may pass closer than `separation` between two knots.
        A lower-priority member yields to a higher one: member 0 plans as if alone, and whether member p finds a way round the
        others is its own round's convergence.  K0 + fleet - 1 <= MAX_OBSTACLES.  obstacle_kinds: the kinds of the caller's K0
        static slots (set_al_obstacles' kinds=); the member spheres behind them are keep-out spheres.  pose_scale: a per-knot
        schedule on the pose weights in batch order (fit_batch's; every round takes its members' rows).  pose_constraints /
        pose_kinds: pose slots in batch order ([K, 4], [B, K, 4] or per knot [B, N+1, K, 4]; al_fit_batch's), every round takes
        its members' rows, and a round that would be a plain fit_batch is an al_fit_batch on them; a family the caller attached
        beforehand (set_al_pose_constraints) is refused.
        Returns (FitResult in batch order, info): min_separation [F] the smallest centre distance over knots and pairs of
        the final plans (inf for fleet = 1), max_violation [B], al_converged [B] int32 (rounds without a constraint: 0 and
        1), outer_iterations [fleet] (python ints)."""
        G = int(fleet)
        if self._pose is not None:
            raise ValueError("plan_fleet under pose constraints the caller attached is not supported (the rounds solve "
                             "sub-batches): detach them with set_al_pose_constraints(None) and give pose_constraints=")
        x0_q, x0_xi = (a if hasattr(a, "shape") else np.asarray(a, dtype=np.float64) for a in (x0_q, x0_xi))
        B = int(x0_q.shape[0])
        if G < 1 or B % G != 0:
            raise ValueError("plan_fleet: B = %d trajectories are not whole fleets of %d" % (B, G))
        if not float(separation) > 0.0:
            raise ValueError("plan_fleet: separation must be positive")
        F = B // G
        q_ref, xi_ref = self._check_refs(B, q_ref, xi_ref) or (None, None)
        if q_ref is None:
            raise ValueError("plan_fleet needs a reference per trajectory: q_ref and xi_ref")
        if obstacles is None and obstacle_kinds is not None:
            raise ValueError("obstacle_kinds describe obstacles: none were given")
        static = None if obstacles is None else self._check_obstacles(B, obstacles, obstacle_kinds)[1]
        if static is not None and static.ndim != 3:
            raise ValueError("plan_fleet: obstacles are static, [K0, 4] or [B, K0, 4]")
        K0 = 0 if static is None else static.shape[1]
        kinds0 = check_kinds(obstacle_kinds, K0)
        if K0 + G - 1 > _capi.MAX_OBSTACLES:
            raise ValueError("plan_fleet: %d spheres + %d other members exceed %d spheres per trajectory"
                             % (K0, G - 1, _capi.MAX_OBSTACLES))
        if pose_constraints is None and pose_kinds is not None:
            raise ValueError("pose_kinds describe pose_constraints: none were given")
        pose = None if pose_constraints is None else self._check_pose_constraints(B, pose_constraints, pose_kinds)[1:]
        if (lb is None) != (ub is None):
            raise ValueError("the input box needs both lb and ub")
        if lb is not None:  # [m], or in batch order [B, m] / [B, N, m]: every round takes its members' rows
            lb, ub = check_input_box(lb, ub, B, self.N, self.m)
        if us_init is None:
            us_init = np.zeros((B, self.N, self.m))
        per = {k: al_kw.pop(k) for k in ("Q", "P", "R") if k in al_kw}
        per["pose_scale"] = self._check_pose_scale(B, pose_scale)
        f64 = dict(dtype=torch.float64, device=self.device)
        maxviol = torch.zeros(B, **f64)
        alconv = torch.ones(B, dtype=torch.int32, device=self.device)
        outers, rounds, pos = [], [], []
        for p in range(G):
            sl = slice(p, None, G)
            kw = dict(q_ref=q_ref[sl], xi_ref=xi_ref[sl], **{k: None if v is None else v[sl] for k, v in per.items()})
            field = [] if static is None else [np.broadcast_to(static[sl][:, None], (F, self.N + 1, K0, 4))]
            for t in pos:  # the members before p: [F, N+1, 3] each
                field.append(np.concatenate([t, np.full((F, self.N + 1, 1), float(separation))], axis=-1)[:, :, None])
            if pose is not None:
                kw.update(pose_constraints=pose[0][sl], pose_kinds=pose[1])
            if not pos and static is None and lb is None and pose is None:
                o = {k: al_kw[k] for k in ("tol_grad_norm", "tol_d_norm", "line_search") if k in al_kw}
                res = self.fit_batch(x0_q[sl], x0_xi[sl], us_init[sl], mode="ms", n_iterations=al_kw.get("n_ilqr_iters", 200),
                                     **o, **kw)
                outers.append(1)
            else:
                obs = np.concatenate(field, axis=2) if pos else None if static is None else static[sl]
                box = (lb, ub) if lb is None or lb.ndim == 1 else (lb[sl], ub[sl])
                res, info = self.al_fit_batch(x0_q[sl], x0_xi[sl], us_init[sl], *box, obstacles=obs,
                                              obstacle_kinds=None if obs is None else kinds0 + (0,) * len(pos), **al_kw, **kw)
                maxviol[sl], alconv[sl] = info["max_violation"], info["al_converged"]
                outers.append(info["outer_iterations"])
            rounds.append(res)
            pos.append(res.xs_q[:, :, :3, 3].cpu().numpy())
        batch = lambda name: torch.stack([getattr(r, name) for r in rounds], dim=1).flatten(0, 1)  # noqa: E731
        out = FitResult(**{n: batch(n) for n in ("xs_q", "xs_xi", "us", "J_hist", "grad_hist", "defect_hist", "alpha_hist",
                                                "mu_hist", "iters", "status", "converged")})
        t = out.xs_q[:, :, :3, 3].reshape(F, G, self.N + 1, 3)
        d = (t[:, :, None] - t[:, None]).norm(dim=-1)                       # [F, G, G, N+1]
        d = d + torch.diag(torch.full((G,), float("inf"), **f64))[None, :, :, None]
        return out, dict(min_separation=d.amin(dim=(1, 2, 3)), max_violation=maxviol, al_converged=alconv,
                         outer_iterations=outers)

    # ------------------------------------------------------------------------------------------
    def linearize_backward(self, xs_q, xs_xi, us, ms=True, mu=1.0, delta=2.0, max_reg=1e10, q_ref=None, xi_ref=None, Q=None,
                           P=None, R=None, pose_scale=None):
        """One _linearization + _backward_pass (+ gradient norm) on given trajectories.  q_ref / xi_ref: a reference per
        trajectory, Q / P / R: weights per trajectory, pose_scale: a per-knot schedule on the pose weights, as for fit_batch
        (rollout / expected_change behind this call use the same references, weights and schedule)."""
        b = self._stage(xs_q, xs_xi, us, (q_ref, xi_ref), (Q, P, R), traj=True, pose_scale=pose_scale)
        B = b.B
        f64 = dict(dtype=torch.float64, device=self.device)
        md = torch.empty(B, 2, **f64)
        md[:, 0] = mu
        md[:, 1] = delta
        r = dict(Fx=torch.empty(B, self.N, 12, 12, **f64), d=torch.empty(B, self.N, 12, **f64),
                 lx=torch.empty(B, self.N + 1, 12, **f64), lxx11=torch.empty(B, self.N + 1, 6, 6, **f64),
                 k=torch.empty(B, self.N, self.m, **f64), K=torch.empty(B, self.N, self.m, 12, **f64),
                 J=torch.empty(B, **f64), dnorm=torch.empty(B, **f64), grad=torch.empty(B, **f64), mu_delta=md)
        self._use_pt(B, b.refs, b.wts, b.sched)
        self._hold(b)
        self._call("tolg_linearize_backward", int(ms), float(max_reg), B, _ptr(b.x_q), _ptr(b.x_xi), _ptr(b.us), _ptr(md),
                   *(_ptr(r[k]) for k in ("Fx", "d", "lx", "lxx11", "k", "K", "J", "dnorm", "grad")), batch=B)
        return r

    def eval_knot(self, i, x_q, x_xi, u=None):
        """Per-knot plugin quantities (f, f_x, f_u, l, l_x, l_xx, l_u, l_uu, err) for n states at knot i."""
        x_q = self._dev(x_q, (-1, 16))
        n = x_q.shape[0]
        x_xi = self._dev(x_xi, (n, 6))
        term = int(i) == self.N
        u_d = None if (u is None or term) else self._dev(u, (n, self.m))
        f64 = dict(dtype=torch.float64, device=self.device)
        r = dict(l=torch.zeros(n, **f64), lx=torch.zeros(n, 12, **f64), lxx=torch.zeros(n, 12, 12, **f64),
                 err=torch.zeros(n, 12, **f64))
        if not term:
            r.update(f_q=torch.zeros(n, 4, 4, **f64), f_xi=torch.zeros(n, 6, **f64), Fx=torch.zeros(n, 12, 12, **f64),
                     Fu=torch.zeros(n, 12, self.m, **f64), lu=torch.zeros(n, self.m, **f64),
                     luu=torch.zeros(n, self.m, self.m, **f64))
        self._call("tolg_eval_knot", int(i), n, _ptr(x_q), _ptr(x_xi), _ptr(u_d),
                   *(_ptr(r.get(k)) for k in ("f_q", "f_xi", "Fx", "Fu", "l", "lx", "lxx", "lu", "luu", "err")))
        return r

    def rollout(self, B, alpha=1.0, ms=True, rollout="nonlinear"):
        """Closed-loop rollout with the gains of the preceding linearize_backward call."""
        f64 = dict(dtype=torch.float64, device=self.device)
        xs_q = torch.empty(B, self.N + 1, 4, 4, **f64)
        xs_xi = torch.empty(B, self.N + 1, 6, **f64)
        us = torch.empty(B, self.N, self.m, **f64)
        self._call("tolg_rollout", int(ms), int(rollout == "linear"), float(alpha), B, _ptr(xs_q), _ptr(xs_xi), _ptr(us))
        return xs_q, xs_xi, us

    def expected_change(self, B, form="auto"):
        """_expected_cost_change of the linear alpha = 1 rollout (traopt_controller.py:2550-2552, :2756-2769) with the
        records and gains of the preceding linearize_backward(ms=True) call.  form: "statement" (the kernel that walks
        the reference's statements), "ring" (the affine recursion alone; flag marks what it hands back, NaN there),
        "auto" (ring + hand-back: what a solve runs).  Returns (ecc [B, 2], flag [B])."""
        ecc = torch.empty(B, 2, dtype=torch.float64, device=self.device)
        flag = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._call("tolg_expected_change", {"statement": 0, "ring": 1, "auto": 2}[form], B, _ptr(ecc), _ptr(flag))
        return ecc, flag

    # ------------------------------------------------------------------------------------------
    def _held_B(self):
        if not self._policy_B:
            raise ValueError("no policy is held: it is left by solve_end / fit_batch / solve_batch_one_call or "
                             "linearize_backward, and cleared by solve_begin and eval_knot")
        return self._policy_B

    def gains(self):
        """The feedback gains of the held policy (what the reference's fit leaves in self._k / self._K): {"k": [B, N, m],
        "K": [B, N, m, 12]} device tensors, in the coordinates of linearize_backward's k / K.  After a solve they are the
        gains of its last backward sweep (about the final trajectory for a converged trajectory, about the iterate before
        it for one stopped by n_iterations); after linearize_backward, about the trajectory it was given."""
        B = self._held_B()
        f64 = dict(dtype=torch.float64, device=self.device)
        k = torch.empty(B, self.N, self.m, **f64)
        K = torch.empty(B, self.N, self.m, 12, **f64)
        self._call("tolg_solve_gains", B, _ptr(k), _ptr(K))
        return {"k": k, "K": K}

    def _check_plant(self, B, plant_J, plant_pend, per_sample):
        """A plant (tolg_set_plant) checked on the host: ValueError before anything reaches the device.  plant_J [B, 6, 6], or
        with per_sample [B, S, 6, 6] too ([..., 3, 3] for so3 and the pendulum: the inertia J_so3, embedded as the model's
        blkdiag(J_so3, I3)); plant_pend [..., 2] = (mass, length), required for the pendulum and refused otherwise.  Each block
        must be finite, symmetric and positive definite, the off-diagonal blocks of a 6x6 zero, the pendulum's parameters
        positive.  Returns None when plant_J is None, else (J [B, S_plant, 36], pend [B, S_plant, 2] or None, form, S_plant)
        with form TOLG_PLANT_DIAG when every off-diagonal entry is zero, TOLG_PLANT_DENSE otherwise."""
        pend_kind = self.problem.kind == "pendulum3d"
        if plant_J is None:
            if plant_pend is not None:
                raise ValueError("plant_pend needs plant_J")
            return None
        n = 3 if self.problem.kind in ("so3", "pendulum3d") else 6
        a = plant_J.detach().cpu().numpy() if isinstance(plant_J, torch.Tensor) else np.asarray(plant_J)
        shape = (B, None, n, n) if per_sample and a.ndim == 4 else (B, n, n)
        a = _checked("plant_J", a, shape, finite=True)
        a = a.reshape(B, -1, n, n)
        Sp = a.shape[1]
        if Sp < 1:
            raise ValueError("plant_J has no samples")
        if n == 3:
            J = np.zeros((B, Sp, 6, 6))
            J[:, :, :3, :3] = a
            J[:, :, 3:, 3:] = np.eye(3)
        else:
            J = a
            if np.any(J[:, :, :3, 3:] != 0.0) or np.any(J[:, :, 3:, :3] != 0.0):
                raise ValueError("plant_J must be blkdiag(Ib, Jv): a non-zero off-diagonal block")
        for blk in (J[:, :, :3, :3], J[:, :, 3:, 3:]):
            if np.any(np.abs(blk - np.swapaxes(blk, -1, -2)) > 1e-12 * np.abs(blk).max(axis=(-1, -2), keepdims=True)):
                raise ValueError("plant_J: the inertia blocks must be symmetric")
            try:
                np.linalg.cholesky(blk)
            except np.linalg.LinAlgError:
                raise ValueError("plant_J: the inertia blocks must be positive definite") from None
        pend = None
        if pend_kind:
            if plant_pend is None:
                raise ValueError("the pendulum's plant needs plant_pend = (mass, length)")
            pend = _checked("plant_pend", plant_pend, (B, Sp, 2) if len(shape) == 4 else (B, 2), finite=True).reshape(B, Sp, 2)
            if np.any(pend <= 0.0):
                raise ValueError("plant_pend: mass and length must be positive")
            pend = np.ascontiguousarray(pend)
        elif plant_pend is not None:
            raise ValueError("plant_pend is for the pendulum only")
        off = J - np.diagonal(J, axis1=-2, axis2=-1)[..., None] * np.eye(6)
        form = _capi.PLANT_DIAG if not np.any(off != 0.0) else _capi.PLANT_DENSE
        return np.ascontiguousarray(J.reshape(B, Sp, 36)), pend, form, Sp

    def _set_plant(self, B, plant):
        """Point the handle at the checked plant (tolg_set_plant; packed into _plant_buf)."""
        J, pend, form, Sp = plant
        d_J, d_pend = self._dev(J, J.shape), None if pend is None else self._dev(pend, pend.shape)
        self._call("tolg_set_plant", B, Sp, form, _ptr(d_J), _ptr(d_pend), *self._packed("_plant_buf", self.lib.tolg_plant_bytes, Sp, B=B))
        return d_J, d_pend

    def _clear_plant(self):
        self._detach("tolg_set_plant")

    def _use_plant(self, B, plant):
        """Point the handle at this call's plant, or detach it (plant None: the model steps): every call states its own.
        Returns the device inputs the stream may not have read yet."""
        if plant is None:
            self._clear_plant()
            return None
        return self._set_plant(B, plant)

    def _box(self, B, u_lb, u_ub):
        """(lb, ub) [B, m] on the device from check_box, or None when neither bound is given."""
        if u_lb is None and u_ub is None:
            return None
        lb, ub = check_box(u_lb, u_ub, B, self.m, so3=self.problem.kind in ("so3", "pendulum3d"))
        return self._dev(lb, (B, self.m)), self._dev(ub, (B, self.m))

    @staticmethod
    def _actuator_struct(box, d_act, delay):
        """The tolg_actuator of a call from its device tensors: box (lb, ub) or None, d_act (beta, du, u_init), each or None."""
        a = _capi.Actuator()
        a.d_lb, a.d_ub = (None, None) if box is None else (box[0].data_ptr(), box[1].data_ptr())
        a.d_beta, a.d_du_max, a.d_u_init = (None if t is None else t.data_ptr() for t in d_act)
        a.delay = int(delay)
        return a

    def _margin_flags(self, clearance, pose_margin, violations):
        """The report keywords of the sampled loops checked against the families attached, ValueError before anything reaches
        the device.  Returns (viol_pos, viol_pose): which counts violations=True fills -- those of every family attached."""
        if clearance and self._obs is None:
            raise ValueError("clearance=True needs keep-out spheres: attach them with set_al_obstacles")
        if pose_margin and self._pose is None:
            raise ValueError("pose_margin=True needs pose constraints: attach them with set_al_pose_constraints")
        if violations and self._obs is None and self._pose is None:
            raise ValueError("violations=True needs a constraint family: attach one with set_al_obstacles or "
                             "set_al_pose_constraints")
        return bool(violations) and self._obs is not None, bool(violations) and self._pose is not None

    def _margin_outputs(self, r, B, S, box, clearance, pose_margin, viol):
        """The report tensors of a sampled loop on r, and their pointers in the order of the C calls: n_sat, u_excess, clear,
        clear_knot, then the four of tolg_policy_rollout_margins."""
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        if box is not None:
            r.n_sat, r.u_excess = torch.empty(B, S, **i32), torch.empty(B, S, **f64)
        if clearance:
            r.clearance, r.clearance_knot = torch.empty(B, S, **f64), torch.empty(B, S, **i32)
        if pose_margin:
            r.pose_margin, r.pose_margin_knot = torch.empty(B, S, **f64), torch.empty(B, S, **i32)
        if viol[0]:
            r.viol_pos = torch.empty(B, self.N + 1, **i32)
        if viol[1]:
            r.viol_pose = torch.empty(B, self.N + 1, **i32)
        return (_ptr(r.n_sat), _ptr(r.u_excess), _ptr(r.clearance), _ptr(r.clearance_knot), _ptr(r.pose_margin),
                _ptr(r.pose_margin_knot), _ptr(r.viol_pos), _ptr(r.viol_pose))

    def policy_rollout(self, dx0=None, noise=None, S=None, trajectories=False, plant_J=None, plant_pend=None, u_lb=None,
                       u_ub=None, clearance=False, pose_margin=False, violations=False, act_tau=None, act_rate=None,
                       act_delay=0, act_u_init=None, commands=False) -> PolicyRollout:
        """S closed-loop rollouts per trajectory of the held policy u = u*_i + K_i (x (-) x*_i) with exact dynamics
        (tolg_policy_rollout).  dx0 [B, S, 12]: start perturbation in the error coordinates of K (pose x*_0 Exp(dx0[:6]),
        twist xi*_0 + dx0[6:]); noise [B, S, N, 6]: added to the twist behind every step.  Either may be None (zero); S is
        taken from them, or given when both are None.  J [B, S] is the tracking cost with the references and weights of the
        held solve (no augmented-Lagrangian terms).  trajectories=True also returns xs_q, xs_xi, us.
        plant_J / plant_pend: the plant the samples are stepped with (model mismatch, tolg_set_plant; None: the model), one per
        sample [B, S, 6, 6] or one per trajectory [B, 6, 6] (see _check_plant).  The cost stays the model's.
        u_lb / u_ub [m] or [B, m] (check_box; both or neither): the actuator's box -- the commanded u*_i + K_i e_i is clamped
        to it before the dynamics step, J and us take the clamped input (tolg_policy_rollout_limited); the result then carries
        n_sat [B, S], how many inputs of the sample the box moved, and u_excess [B, S], the largest distance by which a command
        left it.  clearance=True: the result carries clearance [B, S], min over knots and spheres of |t - c| - r for the
        keep-out spheres attached by set_al_obstacles (negative: the sample entered one; a slot of another kind enters with
        the clearance of its kind, kind_clearance), and clearance_knot, the first knot
        that attains it; ValueError when none are attached.  With none of the three the call is tolg_policy_rollout.
        pose_margin=True: the result carries pose_margin [B, S], min over knots and slots of the margin of the pose slots
        attached by set_al_pose_constraints (pose_margin(): negative, the sample left a cone) and pose_margin_knot, the first
        knot that attains it -- the sampled check of tighten_pose_constraints; ValueError when none are attached.
        violations=True: per knot, how many of the S samples are outside the allowed set there, viol_pos [B, N+1] for the
        position slots and viol_pose [B, N+1] for the pose slots, each when its family is attached (ValueError if neither is):
        viol / S estimates the violation probability a kappa-sigma margin promises at each knot.  rollout_margins() is the
        definition of all four.  With either keyword the call is tolg_policy_rollout_margins.
        act_tau / act_rate / act_delay / act_u_init (check_actuator): the actuator between the command and the step -- a
        transport delay of act_delay knots, the box u_lb / u_ub if given, a first-order lag of time constant act_tau seconds
        and a slew limit of act_rate units per second (include/tolg.h states the model).  `us` and J then take the applied
        input, n_sat / u_excess count on the delayed command, and the result carries n_rate [B, S], the inputs the rate limit
        moved, u_gap [B, S], the largest |applied - commanded| of the sample, and with commands=True u_cmd [B, S, N, m], the
        commands themselves.  With any of the five the call is tolg_policy_rollout_actuated, beside every other keyword; with
        none of them it goes through the entry point it always did."""
        B = self._held_B()
        viol = self._margin_flags(clearance, pose_margin, violations)
        actuated = act_tau is not None or act_rate is not None or act_u_init is not None or commands or \
            isinstance(act_delay, (bool, np.bool_)) or act_delay != 0
        act = None
        if actuated:
            act = check_actuator(u_lb, u_ub, act_tau, act_rate, act_delay, act_u_init, B, self.m, self.problem.dt,
                                 so3=self.problem.kind in ("so3", "pendulum3d"))
            box = None if act[0] is None else (self._dev(act[0], (B, self.m)), self._dev(act[1], (B, self.m)))
        else:
            box = self._box(B, u_lb, u_ub)
        shapes = []
        if dx0 is not None:
            dx0 = _checked("dx0", dx0, (B, None, 12), finite=True)
            shapes.append(dx0.shape[1])
        if noise is not None:
            noise = _checked("noise", noise, (B, None, self.N, 6), finite=True)
            shapes.append(noise.shape[1])
        if S is not None:
            shapes.append(int(S))
        if not shapes:
            raise ValueError("policy_rollout needs S, dx0 or noise")
        if len(set(shapes)) != 1:
            raise ValueError("the sample count differs between dx0, noise and S: %s" % shapes)
        S = shapes[0]
        if S < 1:
            raise ValueError("S must be at least 1")
        plant = self._check_plant(B, plant_J, plant_pend, per_sample=True)
        if plant is not None and plant[3] not in (1, S):
            raise ValueError("plant_J has %d samples per trajectory, the rollout %d" % (plant[3], S))
        f64 = dict(dtype=torch.float64, device=self.device)
        d_dx0 = None if dx0 is None else self._dev(dx0, (B, S, 12))
        d_w = None if noise is None else self._dev(noise, (B, S, self.N, 6))
        r = PolicyRollout(J=torch.empty(B, S, **f64), status=torch.empty(B, S, dtype=torch.int32, device=self.device))
        if trajectories:
            r.xs_q = torch.empty(B, S, self.N + 1, 4, 4, **f64)
            r.xs_xi = torch.empty(B, S, self.N + 1, 6, **f64)
            r.us = torch.empty(B, S, self.N, self.m, **f64)
        limited = box is not None or clearance
        margins = pose_margin or violations
        out = self._margin_outputs(r, B, S, box, clearance, pose_margin, viol)
        d_act = None
        if actuated:
            d_act = tuple(None if a is None else self._dev(a, (B, self.m)) for a in act[2:5])
            i32 = dict(dtype=torch.int32, device=self.device)
            r.n_rate, r.u_gap = torch.empty(B, S, **i32), torch.empty(B, S, **f64)
            if commands:
                r.u_cmd = torch.empty(B, S, self.N, self.m, **f64)
        d_plant = self._use_plant(B, plant)
        try:
            self._hold((d_dx0, d_w, d_plant, box, d_act))
            if actuated:
                a = self._actuator_struct(box, d_act, act[5])
                self._call("tolg_policy_rollout_actuated", B, S, _ptr(d_dx0), _ptr(d_w), C.byref(a), _ptr(r.J), _ptr(r.status),
                           _ptr(r.xs_q), _ptr(r.xs_xi), _ptr(r.us), *out, _ptr(r.u_cmd), _ptr(r.n_rate), _ptr(r.u_gap))
            elif limited or margins:
                lb, ub = box if box is not None else (None, None)
                # (a call with neither new keyword goes through the entry point it always did)
                self._call("tolg_policy_rollout_margins" if margins else "tolg_policy_rollout_limited", B, S, _ptr(d_dx0),
                           _ptr(d_w), _ptr(lb), _ptr(ub), _ptr(r.J), _ptr(r.status), _ptr(r.xs_q), _ptr(r.xs_xi), _ptr(r.us),
                           *(out if margins else out[:4]))
            else:
                self._call("tolg_policy_rollout", B, S, _ptr(d_dx0), _ptr(d_w), _ptr(r.J), _ptr(r.status), _ptr(r.xs_q),
                           _ptr(r.xs_xi), _ptr(r.us))
        finally:
            if plant is not None:
                self._clear_plant()
        return r

    def _stage_moments(self, B, Sigma0, W):
        """Sigma0 and W (either may be None) checked on the host and moved to the device: (d_S0, d_W).  Owns the keep-alive."""
        so3 = self.problem.kind in ("so3", "pendulum3d")
        S0 = None if Sigma0 is None else check_covariance("Sigma0", Sigma0, B, 12, (6, [0, 1, 2, 6, 7, 8]) if so3 else None)
        Wn = None if W is None else check_covariance("W", W, B, 6, (3, [0, 1, 2]) if so3 else None)
        d = (None if S0 is None else self._dev(S0, (B, 12, 12)), None if Wn is None else self._dev(Wn, (B, 6, 6)))
        self._hold(d)
        return d

    def policy_covariance(self, Sigma0=None, W=None, full=False, pos=True) -> PolicyCovariance:
        """The closed-loop covariance of the held policy to first order (tolg_policy_covariance), the analytic companion of
        policy_rollout: Sigma_{i+1} = Acl_i Sigma_i Acl_i^T + E W E^T with Acl_i = f_x + f_u K_i at the held nominal, in the
        error coordinates of K.  Sigma0 [B, 12, 12] or [12, 12] (broadcast): covariance of the start perturbation dx0; W
        [B, 6, 6] or [6, 6]: covariance of the twist disturbance added behind every step; either may be None (zero).  Both are
        checked on the host (check_covariance: shape, finite, symmetric, positive semi-definite).
        so3 and the pendulum: the state is carried in 12 coordinates as in gains() ([rotation, 0, omega, 0]); Sigma0 may also be
        given as [.., 6, 6] over (rotation, omega) and W as [.., 3, 3] over omega -- plant_J's convention for their inertia --
        and are embedded at rows / columns (0..2, 6..8) resp. (0..2); the outputs keep the 12-coordinate layout.
        Returns var_x [B, N+1, 12], var_u [B, N, m], pos_cov [B, N+1, 3, 3] (the world-frame position covariance; pos=False or a
        model without translation: None) and, with full=True, Sigma [B, N+1, 12, 12] (0.95 GB at 4096 x 200).  A plant, an
        input box and keep-out spheres are ignored: the loop is the model's linear, unsaturated one."""
        B = self._held_B()
        d_S0, d_W = self._stage_moments(B, Sigma0, W)
        f64 = dict(dtype=torch.float64, device=self.device)
        r = PolicyCovariance(var_x=torch.empty(B, self.N + 1, 12, **f64), var_u=torch.empty(B, self.N, self.m, **f64))
        if full:
            r.Sigma = torch.empty(B, self.N + 1, 12, 12, **f64)
        pc = torch.empty(B, self.N + 1, 6, **f64) if pos and self.problem.kind not in ("so3", "pendulum3d") else None
        self._call("tolg_policy_covariance", B, _ptr(d_S0), _ptr(d_W), _ptr(r.Sigma), _ptr(r.var_x), _ptr(r.var_u), _ptr(pc))
        if pc is not None:
            iu = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]], device=self.device)
            r.pos_cov = pc[..., iu]
        return r

    def _so3(self):
        return self.problem.kind in ("so3", "pendulum3d")

    def policy_covariance_estimated(self, Sigma0, W, mask, V, full=False, gains=False, pos=True) -> PolicyCovarianceEstimated:
        """The covariance of the held policy under OUTPUT feedback (tolg_policy_covariance_estimated): the loop
        u = u*_i + K_i e^_i acts on the estimate of a Kalman filter that measures the coordinates `mask` of the error state at
        every knot with noise variances V (check_measurement), instead of on the true state as policy_covariance assumes.  With P
        the covariance of the estimation error and S^ that of the estimate's deviation (P_0^- = Sigma0, S^_0^- = 0), at every knot
        Sigma_i = S^- + P^-, the sequential scalar measurement updates give P^+ and the gains L_i[:, j] = P^+[:, j] / V[j],
        S^+ = S^- + (P^- - P^+), and P_{i+1}^- = A_i P^+ A_i^T + E W E^T, S^_{i+1}^- = Acl_i S^+ Acl_i^T (include/tolg.h has the
        statement).  Sigma0 and W as in policy_covariance (either may be None; so3 and the pendulum also in compact form).
        Returns var_x, var_est (diag P^+), var_u, pos_cov [B, N+1, 3, 3] (the shape inflate_obstacles takes; pos=False or a model
        without translation: None); full=True adds Sigma and P_post [B, N+1, 12, 12], gains=True adds L [B, N+1, 12, 12], the
        input of policy_rollout_estimated.  A plant, an input box and constraint geometry are ignored."""
        B = self._held_B()
        m, Vn = check_measurement(mask, V, B, so3=self._so3())
        d_S0, d_W = self._stage_moments(B, Sigma0, W)
        d_V = None if Vn is None else self._dev(Vn, (B, 12))
        self._hold((d_S0, d_W, d_V))
        f64 = dict(dtype=torch.float64, device=self.device)
        n1 = self.N + 1
        r = PolicyCovarianceEstimated(var_x=torch.empty(B, n1, 12, **f64), var_est=torch.empty(B, n1, 12, **f64),
                                      var_u=torch.empty(B, self.N, self.m, **f64), mask=m)
        if full:
            r.Sigma, r.P_post = torch.empty(B, n1, 12, 12, **f64), torch.empty(B, n1, 12, 12, **f64)
        if gains:
            r.L = torch.empty(B, n1, 12, 12, **f64)
        pc = torch.empty(B, n1, 6, **f64) if pos and not self._so3() else None
        self._call("tolg_policy_covariance_estimated", B, _ptr(d_S0), _ptr(d_W), m, _ptr(d_V), _ptr(r.Sigma), _ptr(r.P_post),
                   _ptr(r.L), _ptr(r.var_x), _ptr(r.var_est), _ptr(r.var_u), _ptr(pc))
        if pc is not None:
            iu = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]], device=self.device)
            r.pos_cov = pc[..., iu]
        return r

    def policy_rollout_estimated(self, L, mask, dx0=None, w=None, meas_noise=None, S=None, trajectories=False,
                                 estimates=False, u_lb=None, u_ub=None, clearance=False, pose_margin=False,
                                 violations=False) -> PolicyRollout:
        """S sampled closed loops per trajectory of the held policy under output feedback (tolg_policy_rollout_estimated), the
        Monte-Carlo check of policy_covariance_estimated: the true state starts at x*_0 (+) dx0, the estimate at x*_0; at every
        knot the filter takes y = x (+) meas_noise on the coordinates `mask` and corrects x^ <- x^ (+) L_i r with the residual
        r = [Log(q^^-1 q_y); xi_y - xi^]; the input u = u*_i + K_i e^ is computed from the ESTIMATE and steps both the true state
        (twist noise w added behind the step) and the estimate, on the model's exact dynamics.
        L [B, N+1, 12, 12]: the gains (policy_covariance_estimated(gains=True).L, or the caller's own; columns of unmeasured
        coordinates are not read).  dx0 [B, S, 12], w [B, S, N, 6], meas_noise [B, S, N+1, 12]: each may be None (zero); S is
        taken from them, or given when all are None.  J [B, S] is the tracking cost of the true trajectory and the applied
        inputs.  trajectories=True also returns xs_q, xs_xi, us (the true states); estimates=True est_q, est_xi (the posterior
        estimates).  An attached plant is ignored.
        u_lb / u_ub, clearance, pose_margin, violations: policy_rollout's keywords under its rules
        (tolg_policy_rollout_estimated_limited) -- the input computed from the estimate is clamped to the box and BOTH chains step
        with the clamped input, n_sat / u_excess count it, and clearance, pose margin and the per-knot counts are those of the
        TRUE states, never of the estimates: the check of inflate_obstacles / tighten_pose_constraints fed with the estimated
        loop's covariance.  With none of them the call is tolg_policy_rollout_estimated."""
        B = self._held_B()
        viol = self._margin_flags(clearance, pose_margin, violations)
        box = self._box(B, u_lb, u_ub)
        m = measurement_mask(mask, so3=self._so3())
        if L is None:
            raise ValueError("policy_rollout_estimated needs the gains L [B, N+1, 12, 12]")
        L = _checked("L", L, (B, self.N + 1, 12, 12))
        shapes = []
        if dx0 is not None:
            dx0 = _checked("dx0", dx0, (B, None, 12), finite=True)
            shapes.append(dx0.shape[1])
        if w is not None:
            w = _checked("w", w, (B, None, self.N, 6), finite=True)
            shapes.append(w.shape[1])
        if meas_noise is not None:
            meas_noise = _checked("meas_noise", meas_noise, (B, None, self.N + 1, 12), finite=True)
            shapes.append(meas_noise.shape[1])
        if S is not None:
            shapes.append(int(S))
        if not shapes:
            raise ValueError("policy_rollout_estimated needs S, dx0, w or meas_noise")
        if len(set(shapes)) != 1:
            raise ValueError("the sample count differs between dx0, w, meas_noise and S: %s" % shapes)
        S = shapes[0]
        if S < 1:
            raise ValueError("S must be at least 1")
        f64 = dict(dtype=torch.float64, device=self.device)
        d_L = self._dev(L, (B, self.N + 1, 12, 12))
        d_dx0 = None if dx0 is None else self._dev(dx0, (B, S, 12))
        d_w = None if w is None else self._dev(w, (B, S, self.N, 6))
        d_n = None if meas_noise is None else self._dev(meas_noise, (B, S, self.N + 1, 12))
        r = PolicyRollout(J=torch.empty(B, S, **f64), status=torch.empty(B, S, dtype=torch.int32, device=self.device))
        if trajectories:
            r.xs_q = torch.empty(B, S, self.N + 1, 4, 4, **f64)
            r.xs_xi = torch.empty(B, S, self.N + 1, 6, **f64)
            r.us = torch.empty(B, S, self.N, self.m, **f64)
        if estimates:
            r.est_q = torch.empty(B, S, self.N + 1, 4, 4, **f64)
            r.est_xi = torch.empty(B, S, self.N + 1, 6, **f64)
        out = self._margin_outputs(r, B, S, box, clearance, pose_margin, viol)
        self._hold((d_L, d_dx0, d_w, d_n, box))
        if box is not None or clearance or pose_margin or violations:
            lb, ub = box if box is not None else (None, None)
            self._call("tolg_policy_rollout_estimated_limited", B, S, m, _ptr(d_L), _ptr(d_dx0), _ptr(d_w), _ptr(d_n), _ptr(lb),
                       _ptr(ub), _ptr(r.J), _ptr(r.status), _ptr(r.xs_q), _ptr(r.xs_xi), _ptr(r.us), _ptr(r.est_q),
                       _ptr(r.est_xi), *out)
        else:
            self._call("tolg_policy_rollout_estimated", B, S, m, _ptr(d_L), _ptr(d_dx0), _ptr(d_w), _ptr(d_n), _ptr(r.J),
                       _ptr(r.status), _ptr(r.xs_q), _ptr(r.xs_xi), _ptr(r.us), _ptr(r.est_q), _ptr(r.est_xi))
        return r

    def policy_value(self, Sigma0=None, W=None, full=False) -> PolicyValue:
        """The cost-to-go of the held policy (tolg_policy_value), the backward companion of policy_covariance:
        P_i = M_i + Acl_i^T P_{i+1} Acl_i with M_i = l_xx + K_i^T l_uu K_i and p_i = l_x + K_i^T l_u + Acl_i^T p_{i+1}, from
        P_N = l_xx^N, p_N = l_x^N, with Acl_i = f_x + f_u K_i and the tracking cost's derivatives at the held nominal (the
        model's Jacobians and Gauss-Newton Hessians; trajectory b's own reference and weights where they are set; no
        augmented-Lagrangian terms).  Sigma0 and W as in policy_covariance (checked by check_covariance; so3 and the pendulum
        also in their compact forms): price[b, i] = tr(P_{i+1}[6:12, 6:12] W) / 2 and excess[b] = tr(P_0 Sigma0) / 2 +
        sum_i price[b, i], the expected closed-loop cost above the unperturbed one -- one sweep where policy_rollout needs S
        samples.  Neither P nor p depends on Sigma0 or W.  Returns p [B, N+1, 12], diag_P [B, N+1, 12], price [B, N], excess [B]
        and, with full=True, P [B, N+1, 12, 12] (0.95 GB at 4096 x 200).  A plant, an input box and keep-out spheres are ignored."""
        B = self._held_B()
        d_S0, d_W = self._stage_moments(B, Sigma0, W)
        f64 = dict(dtype=torch.float64, device=self.device)
        r = PolicyValue(p=torch.empty(B, self.N + 1, 12, **f64), diag_P=torch.empty(B, self.N + 1, 12, **f64),
                        price=torch.empty(B, self.N, **f64), excess=torch.empty(B, **f64))
        if full:
            r.P = torch.empty(B, self.N + 1, 12, 12, **f64)
        try:
            self._call("tolg_policy_value", B, _ptr(d_S0), _ptr(d_W), _ptr(r.P), _ptr(r.p), _ptr(r.diag_P), _ptr(r.price),
                       _ptr(r.excess))
        except RuntimeError as e:  # TOLG_E_ARG behind the host's own bookkeeping: the handle's state rules (tolg_solve_gains)
            if "rc=-1" not in str(e):
                raise
            raise ValueError("tolg_policy_value refused the call: the held policy's batch, and the batch per-trajectory "
                             "references and weights are set for, must both be %d" % B) from e
        return r

    # ------------------------------------------------------------------------------------------
    def _paths(self, B, path_q, path_xi):
        """Paths [B, T+1, 4, 4] / [B, T+1, 6] checked on the host and moved to the device as [B, T+1, 16] / [B, T+1, 6];
        returns (q, xi, T)."""
        q = _checked("path_q", path_q, (B, None, 4, 4))
        n = q.shape[1]
        if n < 2:
            raise ValueError("path_q has %d knots, expected T+1 >= 2" % n)
        xi = _checked("path_xi", path_xi, (B, n, 6))
        return self._dev(q, (B, n, 16)), self._dev(xi, (B, n, 6)), n - 1

    def _check_t0(self, B, t0):
        if t0 is None:
            return None
        a = t0.detach().cpu().numpy() if isinstance(t0, torch.Tensor) else np.asarray(t0)
        if a.shape != (B,) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("t0 must be an integer array of shape (%d,)" % B)
        if (a < 0).any() or (a > np.iinfo(np.int32).max).any():
            raise ValueError("t0 must be non-negative int32")
        return torch.as_tensor(a.astype(np.int32), device=self.device)

    def _set_ref_windows(self, B, q, xi, T, t0_d, t):
        self._call("tolg_set_ref_windows", B, _ptr(q), _ptr(xi), int(T), _ptr(t0_d), int(t), *self._packed("_refs_buf", self.lib.tolg_refs_bytes))
        self._refs_set = True

    def set_ref_windows(self, path_q, path_xi, t, t0=None):
        """Point the handle at the windows of B longer paths (tolg_set_ref_windows): trajectory b tracks knots
        min(t0[b] + t + i, T), i = 0..N, of its path, the last knot held past the end.  path_q [B, T+1, 4, 4], path_xi
        [B, T+1, 6], t0 an int array [B] (None: 0).  Like tolg_set_refs it stays set for the calls on this handle that take
        no references of their own (solve_begin / fit_batch without q_ref go back to the shared reference)."""
        B = int(np.shape(path_q)[0]) if len(np.shape(path_q)) else 0
        if not 1 <= B <= self.max_batch:
            raise ValueError("path_q: batch %d outside 1..%d" % (B, self.max_batch))
        if int(t) < 0:
            raise ValueError("t must be non-negative")
        q, xi, T = self._paths(B, path_q, path_xi)
        t0_d = self._check_t0(B, t0)
        self._hold((q, xi, t0_d))
        self._set_ref_windows(B, q, xi, T, t0_d, int(t))

    def _schedule_paths(self, B, path_scale):
        """World-time schedules [B, T+1, 6] checked on the host (finite, not negative, T >= 1) and moved to the device;
        returns (paths, T)."""
        a = _checked("pose_scale_path", path_scale, (B, None, 6), finite=True)
        if a.shape[1] < 2:
            raise ValueError("pose_scale_path has %d knots, expected T+1 >= 2" % a.shape[1])
        if np.any(a < 0.0):
            raise ValueError("pose_scale_path must not be negative")
        return self._dev(a, a.shape), a.shape[1] - 1

    def set_pose_schedule_windows(self, path_scale, t, t0=None):
        """Stage the pose schedule of the next batch call (solve_begin / fit_batch / solve_batch_one_call / al_fit_batch /
        linearize_backward, given no pose_scale of its own) as windows of B longer schedules in world time: path_scale
        [B, T+1, 6]; knot i of trajectory b takes path knot min(t0[b] + t + i, T), set_ref_windows' rule (t0 an int array [B],
        None: 0).  That call gathers the windows on the device behind its weights (tolg_set_pose_schedule_windows) -- the
        schedule sits on per-trajectory weights, and every call states its own -- and is then exactly the call with
        pose_scale= the host-gathered windows; the call after it is unscheduled again.  path_scale = None withdraws what is
        staged."""
        if path_scale is None:
            self._sched_next = None
            return
        B = int(np.shape(path_scale)[0]) if len(np.shape(path_scale)) else 0
        if not 1 <= B <= self.max_batch:
            raise ValueError("path_scale: batch %d outside 1..%d" % (B, self.max_batch))
        if int(t) < 0:
            raise ValueError("t must be non-negative")
        d, T = self._schedule_paths(B, path_scale)
        self._sched_next = (d, T, self._check_t0(B, t0), int(t))

    def mpc_advance(self, w=None, J_cl=None, plant_J=None, plant_pend=None, u_lb=None, u_ub=None, act_tau=None, act_rate=None,
                    act_delay=0, act_state=None):
        """One receding-horizon step on the held policy (tolg_mpc_advance): x_next = f(x*_0, u*_0) + [0; w] with the exact
        dynamics, u = u*_0, and the warm start of the next step (xs_q / xs_xi [B, N+1, ...], us [B, N, m]: the solution
        shifted by one knot, x_next in front, the tail propagated with the last input).  w [B, 6] (None: 0) is added to the
        twist.  J_cl (a float64 device tensor [B], optional) is accumulated with the stage cost l(x*_0, u*_0) at knot 0.
        plant_J [B, 6, 6] / plant_pend [B, 2]: the plant x_next is stepped with (model mismatch, tolg_set_plant; None: the
        model); the warm tail stays the model's prediction, u and J_cl are unchanged.
        u_lb / u_ub [m] or [B, m] (check_box; both or neither): the actuator's box (tolg_mpc_advance_limited) -- u is
        clamp(u*_0), x_next and xs_q[:, 0] step with it, J_cl takes l(x*_0, u); the rest of the warm start is the unclamped
        one, and the dict also holds n_sat [B] int32, the inputs the box moved.
        act_tau / act_rate / act_delay (check_actuator) with act_state: the actuator model between u*_0 and the plant
        (tolg_mpc_advance_actuated) beside the box if one is given.  act_state is a contiguous float64 device tensor
        [B, 1 + act_delay, m] (actuator_state builds the first one from u*_0) and is updated in place: row 0 the last applied
        input, rows 1.. the pending commands, oldest first.  u, x_next, xs_q[:, 0] and J_cl take the applied input; the dict
        also holds n_sat and n_rate [B] int32, the inputs of the step the box / the rate limit moved.
        Returns a dict of device tensors: x_next_q [B, 4, 4], x_next_xi, u [B, m], xs_q, xs_xi, us, J_cl."""
        B = self._held_B()
        actuated = act_tau is not None or act_rate is not None or act_state is not None or \
            isinstance(act_delay, (bool, np.bool_)) or act_delay != 0
        act = None
        if actuated:
            act = self._check_actuated(B, u_lb, u_ub, act_tau, act_rate, act_delay, act_state)
            box = act[0]
        else:
            box = self._box(B, u_lb, u_ub)
        d_w = None if w is None else self._dev(_checked("w", w, (B, 6), finite=True), (B, 6))
        if J_cl is not None and (not isinstance(J_cl, torch.Tensor) or J_cl.dtype != torch.float64 or
                                 tuple(J_cl.shape) != (B,) or J_cl.device != self.device or not J_cl.is_contiguous()):
            raise ValueError("J_cl must be a contiguous float64 tensor of shape (%d,) on %s" % (B, self.device))
        plant = self._check_plant(B, plant_J, plant_pend, per_sample=False)
        r = self._advance_out(B, J_cl, limited=box is not None or actuated, actuated=actuated)
        d_plant = self._use_plant(B, plant)
        try:
            self._hold((d_w, d_plant, box, act))
            self._advance(B, d_w, r, box, act)
        finally:
            if plant is not None:
                self._clear_plant()
        return r

    def _check_actuated(self, B, u_lb, u_ub, act_tau, act_rate, act_delay, act_state, own=False):
        """The actuator of an MPC step checked (check_actuator) and on the device: (box or None, (beta, du, None), delay,
        act_state).  act_state must be the caller's contiguous float64 device tensor [B, 1 + delay, m]; own: the loop's own,
        allocated here and filled by it."""
        lb, ub, beta, du, _, delay = check_actuator(u_lb, u_ub, act_tau, act_rate, act_delay, None, B, self.m, self.problem.dt,
                                                    so3=self.problem.kind in ("so3", "pendulum3d"))
        if own:
            act_state = torch.empty(B, 1 + delay, self.m, dtype=torch.float64, device=self.device)
        if (not isinstance(act_state, torch.Tensor) or act_state.dtype != torch.float64 or
                tuple(act_state.shape) != (B, 1 + delay, self.m) or act_state.device != self.device or
                not act_state.is_contiguous()):
            raise ValueError("act_state must be a contiguous float64 tensor of shape (%d, %d, %d) on %s (actuator_state builds "
                             "one)" % (B, 1 + delay, self.m, self.device))
        box = None if lb is None else (self._dev(lb, (B, self.m)), self._dev(ub, (B, self.m)))
        d_act = tuple(None if a is None else self._dev(a, (B, self.m)) for a in (beta, du)) + (None,)
        return box, d_act, delay, act_state

    def _advance_out(self, B, J_cl, limited=False, actuated=False):
        f64 = dict(dtype=torch.float64, device=self.device)
        more = dict(n_sat=torch.empty(B, dtype=torch.int32, device=self.device)) if limited else {}
        if actuated:
            more["n_rate"] = torch.empty(B, dtype=torch.int32, device=self.device)
        return dict(x_next_q=torch.empty(B, 4, 4, **f64), x_next_xi=torch.empty(B, 6, **f64), u=torch.empty(B, self.m, **f64),
                    xs_q=torch.empty(B, self.N + 1, 4, 4, **f64), xs_xi=torch.empty(B, self.N + 1, 6, **f64),
                    us=torch.empty(B, self.N, self.m, **f64), J_cl=J_cl, **more)

    def _advance(self, B, d_w, r, box=None, act=None):
        out = tuple(_ptr(r[k]) for k in ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us", "J_cl"))
        if act is not None:
            a = self._actuator_struct(act[0], act[1], act[2])
            self._call("tolg_mpc_advance_actuated", B, _ptr(d_w), C.byref(a), _ptr(act[3]), *out, _ptr(r["n_sat"]),
                       _ptr(r["n_rate"]))
        elif box is None:
            self._call("tolg_mpc_advance", B, _ptr(d_w), *out)
        else:
            self._call("tolg_mpc_advance_limited", B, _ptr(d_w), _ptr(box[0]), _ptr(box[1]), *out, _ptr(r["n_sat"]))

    def mpc_measure(self, mask, V, x_q, x_xi, est_q, est_xi, P, noise=None, gains=True):
        """The filter's update at one world knot (tolg_mpc_measure): y = x (+) noise is measured on the coordinates `mask` with
        variances V (check_measurement), the sequential scalar updates take P to P^+, L[:, j] = P^+[:, j] / V[j], and the estimate
        becomes x^ (+) L r with the residual r = [Log(q^^-1 q_y); xi_y - xi^] on the measured coordinates.  x_q [B, 4, 4] (or
        [B, 16]) and x_xi [B, 6]: the true state; est_q, est_xi, P [B, 12, 12]: the caller's contiguous float64 device tensors,
        updated in place (check_owned; prior in, posterior out, P mirrored from its upper triangle).  noise [B, 12] or None.
        Needs no held policy and is legal during a solve in flight.  Returns a dict of device tensors: innov [B, 12], var_est
        [B, 12] and, with gains=True, L [B, 12, 12]."""
        if not isinstance(est_xi, torch.Tensor) or est_xi.ndim != 2:
            raise ValueError("est_xi must be a contiguous float64 tensor of shape (B, 6) on %s" % (self.device,))
        B = est_xi.shape[0]
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d outside 1..%d" % (B, self.max_batch))
        m, Vn = check_measurement(mask, V, B, so3=self._so3())
        for name, t, shapes in (("x_q", x_q, ((B, 4, 4), (B, 16))), ("x_xi", x_xi, ((B, 6),)), ("est_q", est_q, ((B, 4, 4), (B, 16))),
                                ("est_xi", est_xi, ((B, 6),)), ("P", P, ((B, 12, 12),))):
            check_owned(name, t, shapes, self.device)
        d_V = None if Vn is None else self._dev(Vn, (B, 12))
        d_n = None if noise is None else self._dev(_checked("noise", noise, (B, 12), finite=True), (B, 12))
        f64 = dict(dtype=torch.float64, device=self.device)
        r = dict(innov=torch.empty(B, 12, **f64), var_est=torch.empty(B, 12, **f64), L=torch.empty(B, 12, 12, **f64) if gains else None)
        self._meas_inflight = (d_V, d_n)  # (a keep-alive of its own: a solve in flight keeps its inputs in the other)
        self._measure(B, m, d_V, x_q, x_xi, d_n, est_q, est_xi, P, r["L"], r["innov"], r["var_est"])
        return r

    def _measure(self, B, m, d_V, x_q, x_xi, d_n, est_q, est_xi, P, L, innov, var_est):
        self._call("tolg_mpc_measure", B, m, _ptr(d_V), _ptr(x_q), _ptr(x_xi), _ptr(d_n), _ptr(est_q), _ptr(est_xi), _ptr(P),
                   _ptr(L), _ptr(innov), _ptr(var_est))

    def mpc_advance_estimated(self, x_true_q, x_true_xi, P, w=None, W=None, J_cl=None, plant_J=None, plant_pend=None, u_lb=None,
                              u_ub=None):
        """One receding-horizon step of a loop that acts on an estimate (tolg_mpc_advance_estimated): the held policy's solve
        began from the filter's posterior, so x*_0 is that estimate.  u = clamp(u*_0) (u_lb / u_ub as mpc_advance; both or
        neither).  The TRUE state x_true_q [B, 4, 4] (or [B, 16]), x_true_xi [B, 6] steps in place with u -- on the plant
        (plant_J / plant_pend, as mpc_advance) where one is given, else on the model -- and takes the twist disturbance w
        [B, 6]; x_next = f(x*_0, u) on the model without w is the estimate's prior and xs_q[:, 0]; P [B, 12, 12] becomes
        A P A^T + E W E^T in place with A = f_x(x*_0, u*_0) and W [6, 6] or [B, 6, 6] (check_covariance; None: 0).  J_cl is
        accumulated with the stage cost of the true state before the step.  x_true_q, x_true_xi and P are the caller's
        contiguous float64 device tensors (check_owned).  No actuator model: output feedback behind one is out of scope.
        Returns mpc_advance's dict (x_next_q, x_next_xi, u, xs_q, xs_xi, us, J_cl, n_sat)."""
        B = self._held_B()
        for name, t, shapes in (("x_true_q", x_true_q, ((B, 4, 4), (B, 16))), ("x_true_xi", x_true_xi, ((B, 6),)),
                                ("P", P, ((B, 12, 12),))):
            check_owned(name, t, shapes, self.device)
        box = self._box(B, u_lb, u_ub)
        d_w = None if w is None else self._dev(_checked("w", w, (B, 6), finite=True), (B, 6))
        d_W = None if W is None else self._dev(check_covariance("W", W, B, 6, (3, [0, 1, 2]) if self._so3() else None), (B, 6, 6))
        if J_cl is not None:
            check_owned("J_cl", J_cl, ((B,),), self.device)
        plant = self._check_plant(B, plant_J, plant_pend, per_sample=False)
        r = self._advance_out(B, J_cl, limited=True)
        d_plant = self._use_plant(B, plant)
        try:
            self._hold((d_w, d_W, d_plant, box))
            self._advance_est(B, d_w, box, x_true_q, x_true_xi, P, d_W, r)
        finally:
            if plant is not None:
                self._clear_plant()
        return r

    def _measure_step(self, B, est, t, res):
        """The loop's measure at world knot t on its own buffers (est: mpc()'s dict), recorded in res."""
        self._measure(B, est["mask"], est["V"], est["xt_q"], est["xt_xi"], None if est["n"] is None else est["n"][t], est["e_q"],
                      est["e_xi"], est["P"], None, est["innov"], est["var"])
        res.est_q[:, t] = est["e_q"].reshape(B, 4, 4)
        res.est_xi[:, t] = est["e_xi"]
        res.est_var[:, t] = est["var"]
        res.innov[:, t] = est["innov"]

    def _advance_est(self, B, d_w, box, x_true_q, x_true_xi, P, d_W, r):
        out = tuple(_ptr(r[k]) for k in ("x_next_q", "x_next_xi", "u", "xs_q", "xs_xi", "us", "J_cl"))
        lb, ub = box if box is not None else (None, None)
        self._call("tolg_mpc_advance_estimated", B, _ptr(d_w), _ptr(lb), _ptr(ub), _ptr(x_true_q), _ptr(x_true_xi), _ptr(P),
                   _ptr(d_W), *out, _ptr(r["n_sat"]))

    def mpc(self, x0_q, x0_xi, path_q, path_xi, steps, us_init=None, t0=None, iters_per_step=5, first_iters=50,
            warm="states", noise=None, mode="ms", line_search=False, rollout="nonlinear", tol_grad_norm=1e-6, tol_d_norm=1e-6,
            check_every=0, Q=None, P=None, R=None, max_reg=1e10, on_step=None, plant_J=None, plant_pend=None, u_lb=None,
            u_ub=None, lb=None, ub=None, lb_path=None, ub_path=None, obstacles=None, obstacle_paths=None, obstacle_kinds=None, first_al_iters=3,
            al_iters_per_step=1, mu0=1e-2, mu_scale=10.0, mu_max=1e8, tol_constr=1e-2, pose_scale_path=None,
            pose_constraints=None, pose_paths=None, pose_kinds=None, act_tau=None, act_rate=None, act_delay=0, meas_mask=None,
            meas_V=None, meas_noise=None, est_Sigma0=None, est_W=None, est_dx0=None) -> MPCResult:
        """Receding-horizon MPC: `steps` closed-loop steps of B trajectories, each tracking its own path from its own phase.
        Step t: windows min(t0[b] + t + i, T) of the paths (tolg_set_ref_windows), a solve of first_iters (t = 0) or
        iters_per_step iterations, then tolg_mpc_advance applies u*_0, steps the plant with the exact dynamics and adds the
        twist disturbance noise[:, t] ([B, steps, 6], None: 0).  The next solve starts from the measured state and
          warm="states":   the previous solution shifted by one knot, states and controls (tolg_solve_begin_warm; MS only);
          warm="controls": the shifted controls only, MS states from the reference window (tolg_solve_begin).
        The first solve starts from us_init (None: 0) and the reference window.  check_every = 0 issues a fixed count of
        iterations with no host read in the whole loop; > 0 stops a step's solve early (solve_iterate_until).  Q / P / R:
        weights per trajectory as for fit_batch.  pose_scale_path [B, T_s+1, 6]: a schedule on the pose weights in world time,
        gathered every step with the same t0 as the reference windows (tolg_set_pose_schedule_windows; without Q / P / R on the
        problem's own weights); the handle is left without one.  on_step(t, FitResult) is called behind every step's solve (before the
        plant step; the FitResult carries histories then).  plant_J [B, 6, 6] / plant_pend [B, 2]: the plant every step's
        x_next is stepped with (model mismatch, as mpc_advance; None: the model); the solves plan on the model.  u_lb / u_ub [m] or
        [B, m]: the actuator's box (as mpc_advance: every step applies clamp(u*_0); it clips the plant only and is independent
        of the planner's lb / ub), the result then carries n_sat [B, steps].  act_tau / act_rate / act_delay (check_actuator):
        the actuator model between every step's u*_0 and the plant (as mpc_advance; the loop owns the actuator's state across
        the steps, at rest on the first step's u*_0), beside the box, the planner's constraints and the plant; `us` holds the
        applied inputs and the result carries n_sat and n_rate [B, steps].  Not with an
        augmented-Lagrangian constraint the caller attached.  The handle is left on the shared reference and weights, without a
        plant, with no constraint attached.
        x0_q [B, 4, 4], x0_xi [B, 6], path_q [B, T+1, 4, 4], path_xi [B, T+1, 6].
        The planner's constraints (augmented Lagrangian, mode="ms" only; with none of them the loop is the one above): lb / ub
        [m], the input box of set_al (the SO3 family takes the box only), or a box per trajectory [B, m], or [B, N, m], per
        knot and fixed in window coordinates (knot i of every step's window; check_input_box), or lb_path / ub_path
        [B, T_b+1, m], boxes in world time indexed with the same t0 (window t is gathered by tolg_set_al_box_windows; the
        static pair or the path pair, never both; the plant's u_lb / u_ub are another matter: they clip, these plan); obstacles [K, 4] or [B, K, 4], static keep-out
        spheres, or obstacle_paths [B, T_o+1, K, 4], spheres in world time indexed with the same t0 (window t is gathered by
        tolg_set_al_obstacle_windows); at most one of the two; obstacle_kinds: the kind of each of their K slots
        (set_al_obstacles' kinds=; the clearance is then each kind's own); pose_constraints [K, 4] or [B, K, 4], static pose slots
        (tilt cones, view cones: set_al_pose_constraints), or pose_paths [B, T_p+1, K, 4], pose slots in world time indexed with
        the same t0 (window t is gathered by tolg_set_al_pose_constraint_windows); at most one of the two, pose_kinds with
        either; alone or beside the others, not for the SO3 family; the rounds then end in tolg_al_mpc_step_pose.  Step t then runs first_al_iters (t = 0) or al_iters_per_step
        outer rounds: each a solve as above followed by tolg_al_mpc_step, which shifts the multipliers by one knot behind the
        step's last round; round 0 starts as above, round a > 0 from round a-1's solution under the `warm` rule.  The
        multipliers start at lambda = 0, I_mu = mu = mu0 (mu_scale, mu_max, tol_constr: al_fit_batch's).  The result carries
        max_violation [B, steps] (each step's last round), mu [B] and, with spheres, clearance [B, steps+1] of the realised
        states, with pose slots pose_margin [B, steps+1], the smallest pose_margin() of each realised state under the slots of
        its world knot t0[b] + s (pose_paths: held past the path's end).  iters and status are those of each step's last round.
        Output feedback (any of meas_mask, meas_V, meas_noise, est_Sigma0, est_W, est_dx0; check_mpc_estimated): the loop acts
        on the estimate of a Kalman filter carried from step to step instead of on the plant's exact state.  x0 is then what the
        vehicle BELIEVES, the filter's prior with covariance est_Sigma0 ([12, 12] or [B, 12, 12], None: 0); the true state starts
        at x0 (+) est_dx0 ([B, 12], None: 0).  Step t: the windows are set; tolg_mpc_measure takes y = x_true (+) meas_noise[:, t]
        ([B, steps+1, 12], None: 0) on the coordinates meas_mask with variances meas_V ([12] or [B, 12]); the solve starts from
        the posterior (its x0 and, for warm="states", xs_warm[:, 0]); the AL rounds, if any; tolg_mpc_advance_estimated steps the
        true state with clamp(u*_0) on the plant and adds noise[:, t], steps the estimate on the model and P <- A P A^T + E est_W
        E^T (est_W [6, 6] or [B, 6, 6], None: 0).  One more measure follows the last step.  xs_q, xs_xi, J, clearance and
        pose_margin are those of the TRUE states; the result also carries est_q, est_xi, est_var (diag P^+) and innov, steps+1
        entries each.  It composes with plant_*, u_lb / u_ub and the planner's constraints, and raises ValueError with act_*
        (output feedback behind an actuator model is out of scope).  No host read in the loop.  on_step's FitResult also carries
        extra["est_P"] [B, 12, 12], the posterior covariance of the step (the loop's own buffer: copy it to keep it)."""
        if self._al is not None:
            raise ValueError("mpc under an augmented-Lagrangian constraint is not supported: detach it with set_al(None)")
        if self._obs is not None:
            raise ValueError("mpc with keep-out spheres is not supported: detach them with set_al_obstacles(None)")
        if self._pose is not None:
            raise ValueError("mpc with pose constraints is not supported: detach them with set_al_pose_constraints(None)")
        if warm not in ("states", "controls"):
            raise ValueError("warm must be 'states' or 'controls'")
        if mode not in ("ms", "ss"):
            raise ValueError("mode must be 'ms' or 'ss'")
        if warm == "states" and mode != "ms":
            raise ValueError("warm='states' warm-starts the shooting states of multiple shooting; use warm='controls' "
                             "with mode='ss'")
        steps, K0, K = int(steps), int(first_iters), int(iters_per_step)
        if steps < 1 or K0 < 0 or K < 0 or int(check_every) < 0:
            raise ValueError("steps must be >= 1, first_iters, iters_per_step and check_every >= 0")
        if (lb is None) != (ub is None):
            raise ValueError("the input box needs both lb and ub")
        if (lb_path is None) != (ub_path is None):
            raise ValueError("the input box in world time needs both lb_path and ub_path")
        if lb is not None and lb_path is not None:
            raise ValueError("give lb / ub (fixed in window coordinates) or lb_path / ub_path (world time), not both")
        if obstacles is not None and obstacle_paths is not None:
            raise ValueError("give obstacles (static) or obstacle_paths (world time), not both")
        if obstacle_kinds is not None and obstacles is None and obstacle_paths is None:
            raise ValueError("obstacle_kinds describe obstacles: none were given")
        if pose_constraints is not None and pose_paths is not None:
            raise ValueError("give pose_constraints (static) or pose_paths (world time), not both")
        if pose_kinds is not None and pose_constraints is None and pose_paths is None:
            raise ValueError("pose_kinds describe pose_constraints or pose_paths: none were given")
        posed = pose_constraints is not None or pose_paths is not None
        constrained = lb is not None or lb_path is not None or obstacles is not None or obstacle_paths is not None or posed
        if constrained and mode != "ms":
            raise ValueError("the augmented-Lagrangian constraints need mode='ms'")
        if constrained and (int(first_al_iters) < 1 or int(al_iters_per_step) < 1):
            raise ValueError("first_al_iters and al_iters_per_step must be >= 1")
        x0_q = _checked("x0_q", x0_q, (None, 16) if np.ndim(x0_q) == 2 else (None, 4, 4))
        B = x0_q.shape[0]
        if not 1 <= B <= self.max_batch:
            raise ValueError("batch %d outside 1..%d" % (B, self.max_batch))
        x0_xi = _checked("x0_xi", x0_xi, (B, 6))
        if us_init is not None:
            us_init = _checked("us_init", us_init, (B, self.N, self.m))
        pq, pxi, T = self._paths(B, path_q, path_xi)
        t0_d = self._check_t0(B, t0)
        self._sched_next = None  # the loop's schedule is pose_scale_path
        b = self._stage(x0_q, x0_xi, us_init, weights=(Q, P, R))
        spath = None if pose_scale_path is None else self._schedule_paths(B, pose_scale_path)
        if spath is not None and b.wts is None:
            b.wts = tuple(self._dev(a, a.shape) for a in self._own_weights(B))
        plant = self._check_plant(B, plant_J, plant_pend, per_sample=False)
        actuated = act_tau is not None or act_rate is not None or isinstance(act_delay, (bool, np.bool_)) or act_delay != 0
        act = None
        if actuated:  # (the state is filled from the first step's u*_0, behind its solve)
            act = self._check_actuated(B, u_lb, u_ub, act_tau, act_rate, act_delay, None, own=True)
            box = act[0]
        else:
            box = self._box(B, u_lb, u_ub)
        if noise is not None:
            noise = _checked("noise", noise, (B, steps, 6), finite=True)
            noise = self._dev(np.ascontiguousarray(noise.transpose(1, 0, 2)), (steps, B, 6))  # step t: one contiguous [B, 6]
        f64 = dict(dtype=torch.float64, device=self.device)
        est = None
        if any(a is not None for a in (meas_mask, meas_V, meas_noise, est_Sigma0, est_W, est_dx0)):
            em, eV, en, eS0, eW, edx = check_mpc_estimated(B, steps, self._so3(), meas_mask, meas_V, meas_noise, est_Sigma0, est_W,
                                                           est_dx0, actuated=actuated)
            est = dict(mask=em, V=None if eV is None else self._dev(eV, (B, 12)),
                       n=None if en is None else self._dev(en, (steps + 1, B, 12)), P=self._dev(eS0, (B, 12, 12)),
                       W=None if eW is None else self._dev(eW, (B, 6, 6)),
                       # the true state, stepped in place by tolg_mpc_advance_estimated; the estimate, updated in place by the measure
                       xt_q=b.x_q.reshape(B, 16).clone(), xt_xi=b.x_xi.clone(), e_q=b.x_q.reshape(B, 16).clone(), e_xi=b.x_xi.clone())
            if edx is not None:
                tq, txi = perturbed_state(b.x_q.reshape(B, 4, 4).cpu().numpy(), b.x_xi.cpu().numpy(), edx)
                est["xt_q"], est["xt_xi"] = self._dev(tq, (B, 16)), self._dev(txi, (B, 6))
        # the planner's constraints, checked before anything is attached: (lb, ub, lam, imu), (geometry, lam, imu, in world time)
        al = obs = pose = mu = maxviol = None
        if posed:  # (slots, lam, imu, in world time, kinds)
            slots, pkinds = (self._check_pose_constraints(B, pose_constraints, pose_kinds)[1:] if pose_constraints is not None else
                             self._check_pose_paths(B, pose_paths, pose_kinds)[1:])
            if pose_constraints is not None and slots.ndim != 3:
                raise ValueError("mpc: pose_constraints are static, [K, 4] or [B, K, 4]; slots that move are pose_paths")
            Kp = slots.shape[-2]
            pose = (self._dev(slots, slots.shape), torch.zeros(B, self.N + 1, Kp, **f64),
                    torch.full((B, self.N + 1, Kp), float(mu0), **f64), pose_paths is not None, pkinds)
        if lb is not None or lb_path is not None:  # (lb, ub, lam, imu, in world time)
            if lb_path is not None:
                if self._so3() or self.problem.kind == "pendulum3d":
                    raise ValueError("mpc: lb_path / ub_path are not offered for the %s model" % self.problem.kind)
                lo, hi = self._box_paths(B, lb_path, ub_path)
            else:
                lo, hi = check_input_box(lb, ub, B, self.N, self.m)  # (on the host: set_al uploads them, once)
            al = (lo, hi, torch.zeros(B, self.N, 2 * self.m, **f64), torch.full((B, self.N, 2 * self.m), float(mu0), **f64),
                  lb_path is not None)
        if obstacles is not None or obstacle_paths is not None:
            geo = (self._check_obstacles(B, obstacles, obstacle_kinds)[1] if obstacles is not None else
                   self._check_obstacle_paths(B, obstacle_paths, obstacle_kinds)[1])
            if obstacles is not None and geo.ndim != 3:
                raise ValueError("mpc: obstacles are static, [K, 4] or [B, K, 4]; spheres that move are obstacle_paths")
            Ko = geo.shape[-2]
            kinds = check_kinds(obstacle_kinds, Ko)
            obs = (self._dev(geo, geo.shape), torch.zeros(B, self.N + 1, Ko, **f64),
                   torch.full((B, self.N + 1, Ko), float(mu0), **f64), obstacle_paths is not None)
        if constrained:
            mu, maxviol = torch.full((B,), float(mu0), **f64), torch.empty(B, **f64)
        res = MPCResult(xs_q=torch.empty(B, steps + 1, 4, 4, **f64), xs_xi=torch.empty(B, steps + 1, 6, **f64),
                        us=torch.empty(B, steps, self.m, **f64), J=torch.zeros(B, **f64),
                        iters=torch.empty(B, steps, dtype=torch.int32, device=self.device),
                        status=torch.empty(B, steps, dtype=torch.int32, device=self.device))
        res.xs_q[:, 0] = b.x_q.reshape(B, 4, 4)
        res.xs_xi[:, 0] = b.x_xi
        if est is not None:
            res.xs_q[:, 0], res.xs_xi[:, 0] = est["xt_q"].reshape(B, 4, 4), est["xt_xi"]
            res.est_q, res.est_xi = torch.empty(B, steps + 1, 4, 4, **f64), torch.empty(B, steps + 1, 6, **f64)
            res.est_var, res.innov = torch.empty(B, steps + 1, 12, **f64), torch.empty(B, steps + 1, 12, **f64)
            est["var"], est["innov"] = torch.empty(B, 12, **f64), torch.empty(B, 12, **f64)
        # the plant state and the warm start: written by tolg_mpc_advance, read by the next begin (stream-ordered)
        adv = self._advance_out(B, res.J, limited=box is not None or actuated or est is not None, actuated=actuated)
        if box is not None or actuated:
            res.n_sat = torch.empty(B, steps, dtype=torch.int32, device=self.device)
        if actuated:
            res.n_rate = torch.empty(B, steps, dtype=torch.int32, device=self.device)
        x_q, x_xi, us = b.x_q, b.x_xi, b.us
        try:
            # the plant survives the solves of the loop (tolg_set_plant): set once, detached behind it
            d_plant = self._use_plant(B, plant)
            self._hold((b, pq, pxi, t0_d, noise, adv, d_plant, box, al, obs, pose, mu, maxviol, spath, act, est))
            self._use_pt(B, None, b.wts)
            if al is not None and not al[4]:
                self.set_al(*al[:4])
            if obs is not None and not obs[3]:
                self.set_al_obstacles(*obs[:3], kinds)
            if pose is not None and not pose[3]:
                self.set_al_pose_constraints(pose[0], pose[4], pose[1], pose[2])
            if constrained:
                res.max_violation, res.mu = torch.empty(B, steps, **f64), mu
            for t in range(steps):
                self._set_ref_windows(B, pq, pxi, T, t0_d, t)
                if spath is not None:
                    self._set_pose_schedule(B, (spath[0], spath[1], t0_d, t))
                if al is not None and al[4]:
                    self._set_box_windows(B, al[0], al[1], t0_d, t, al[2], al[3])
                if obs is not None and obs[3]:
                    self._set_obstacle_windows(B, obs[0], t0_d, t, obs[1], obs[2], kinds)
                if pose is not None and pose[3]:
                    self._set_pose_windows(B, pose[0], t0_d, t, pose[1], pose[2], pose[4])
                n = K0 if t == 0 else K
                o = self._options(mode, n, line_search, rollout, tol_grad_norm, tol_d_norm, max_reg)
                xs = None
                if t > 0:
                    x_q, x_xi = adv["x_next_q"].reshape(B, 16), adv["x_next_xi"]
                    us = adv["us"]
                    if warm == "states":
                        xs = (adv["xs_q"].reshape(B, self.N + 1, 16), adv["xs_xi"])
                if est is not None:  # the filter's update at world knot t; the solve starts from the posterior
                    if t > 0:
                        est["e_q"].copy_(x_q)
                        est["e_xi"].copy_(x_xi)
                    self._measure_step(B, est, t, res)
                    x_q, x_xi = est["e_q"], est["e_xi"]
                    if xs is not None:
                        xs[0][:, 0] = x_q
                        xs[1][:, 0] = x_xi
                rounds = (int(first_al_iters) if t == 0 else int(al_iters_per_step)) if constrained else 1
                for a in range(rounds):
                    if a > 0:  # from the round before, under the rule of `warm`
                        us = out.us
                        xs = (out.xs_q.reshape(B, self.N + 1, 16), out.xs_xi) if warm == "states" else None
                    out = self._alloc_result(B, n, histories=on_step is not None)
                    self._begin(o, B, x_q, x_xi, us, xs, out)
                    if check_every:
                        self.solve_iterate_until(n, int(check_every))
                    else:
                        self.solve_iterate(n)
                    out = self.solve_end()
                    if constrained:
                        self._al_step(B, out.xs_q, out.us, mu, mu_scale, mu_max, tol_constr, maxviol, a == rounds - 1)
                if constrained:
                    res.max_violation[:, t] = maxviol
                res.iters[:, t] = out.iters
                res.status[:, t] = out.status
                if on_step is not None:
                    if est is not None:  # the filter's posterior covariance of this step: the loop's own buffer, copy to keep
                        out.extra["est_P"] = est["P"]
                    on_step(t, out)
                if actuated and t == 0:  # at rest on the first command
                    act[3][:] = out.us[:, 0, None, :]
                if est is not None:
                    self._advance_est(B, None if noise is None else noise[t], box, est["xt_q"], est["xt_xi"], est["P"], est["W"], adv)
                else:
                    self._advance(B, None if noise is None else noise[t], adv, box, act)
                if box is not None or actuated:
                    res.n_sat[:, t] = adv["n_sat"]
                if actuated:
                    res.n_rate[:, t] = adv["n_rate"]
                res.us[:, t] = adv["u"]
                if est is not None:
                    res.xs_q[:, t + 1] = est["xt_q"].reshape(B, 4, 4)
                    res.xs_xi[:, t + 1] = est["xt_xi"]
                else:
                    res.xs_q[:, t + 1] = adv["x_next_q"]
                    res.xs_xi[:, t + 1] = adv["x_next_xi"]
            if est is not None:  # one more measure behind the last step: steps + 1 estimates
                est["e_q"].copy_(adv["x_next_q"].reshape(B, 16))
                est["e_xi"].copy_(adv["x_next_xi"])
                self._measure_step(B, est, steps, res)
            if obs is not None:  # the realised state s of trajectory b is at world knot t0[b] + s
                geo = obs[0]
                if obs[3]:
                    s = torch.arange(steps + 1, device=self.device)[None, :] + (0 if t0_d is None else t0_d.long()[:, None])
                    geo = geo[torch.arange(B, device=self.device)[:, None], s.clamp(max=geo.shape[1] - 1).expand(B, steps + 1)]
                else:
                    geo = geo[:, None]
                if any(kinds):
                    d = kind_clearance(res.xs_q[:, :, :3, 3], geo, kinds)
                else:
                    d = (res.xs_q[:, :, None, :3, 3] - geo[..., :3]).norm(dim=-1) - geo[..., 3]
                res.clearance = d.amin(dim=-1)
            if pose is not None:  # likewise: on the device tensors, the slots of world knot t0[b] + s
                geo = pose[0]
                if pose[3]:
                    s = torch.arange(steps + 1, device=self.device)[None, :] + (0 if t0_d is None else t0_d.long()[:, None])
                    geo = geo[torch.arange(B, device=self.device)[:, None], s.clamp(max=geo.shape[1] - 1).expand(B, steps + 1)]
                else:
                    geo = geo[:, None]
                res.pose_margin = pose_margin(res.xs_q, geo, pose[4]).amin(dim=-1)
        finally:
            self._use_pt(B, None, None)
            if plant is not None:
                self._clear_plant()
            if self._al is not None:
                self.set_al(None)
            if self._obs is not None:
                self.set_al_obstacles(None)
            if self._pose is not None:
                self.set_al_pose_constraints(None)
        return res

    # ------------------------------------------------------------------------------------------
    def enable_timing(self, on=True):
        self.lib.tolg_enable_timing(self._h, int(on))

    def kernel_time(self, reset=True):
        """(ms in backward sweeps, ms in rollouts, ms in linearisation, number of backward launches)
        measured with HIP events on the launch stream."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self.lib.tolg_kernel_time(self._h, int(reset), C.byref(a), C.byref(b), C.byref(c), C.byref(n))
        return a.value, b.value, c.value, n.value
