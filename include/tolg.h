/*
 * tolg.h -- C ABI of libtolg_hip.so: batched tracking-iLQR on SE(3) for MI355X (gfx950).
 *
 * This is the drop-in boundary for the hot path of
 * chenghuailin/trajectory_optimization_matrix_lie_groups.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root).  The reference is pure
 * Python (no FFI of its own); the binding a maintainer adds is the ctypes stub shown in
 * INTEGRATION.md -- exactly what trajectory_optimization_matrix_lie_groups_amd/_capi.py does.
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory owned by the caller (PyTorch-ROCm tensors);
 *     the library never allocates, frees or synchronises; all work is enqueued on `stream`
 *     (a hipStream_t passed as void*).
 *   - poses are 4x4 row-major homogeneous matrices, twists are [omega, v]
 *     (traoptlibrary/traopt_utilis.py:43-92), fp64 throughout.
 *   - return value: 0 ok, <0 argument / launch error (TOLG_E_*); per-trajectory outcomes are
 *     written to d_status[B] (TOLG_ST_*).  No exception crosses this boundary.
 */
#ifndef TOLG_H
#define TOLG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* TOLG_DYN_SO3: SO3Dynamics / SO3TrackingQuadraticGaussNewtonCost / iLQR_Tracking_SO3{,_MS}
 * (traoptlibrary/traopt_dynamics.py:275-418, traopt_cost.py:280-564, traopt_controller.py:526-1824)
 * carried in the SE(3) layout: poses are 4x4 with zero translation, twists [omega, 0], m = 6 with
 * u[3:6] = 0, J = blkdiag(J_so3, I3), R = blkdiag(R_so3, I3), Q/P with zero rows for the unused
 * coordinates.  The rotational sub-problem decouples exactly; Jacobian and cost follow the SO3
 * classes (no swapped-twist quirk, terminal l and l_x weighted with Q). */
/* TOLG_DYN_PENDULUM3D: Pendulum3dDyanmics (traoptlibrary/traopt_dynamics.py:421-626) under the SO3 cost and
 * controllers, same embedding as TOLG_DYN_SO3; the pivot acceleration u in R^3 is u[0:3].  Its F_u
 * depends on the state (J^-1 skew(m rho) R^T dt), the lower-left block of F_x on the input. */
enum { TOLG_DYN_SE3 = 0, TOLG_DYN_RIGIDBODY = 1, TOLG_DYN_DRONE = 2, TOLG_DYN_SO3 = 3, TOLG_DYN_PENDULUM3D = 4 };
enum { TOLG_MODE_MS = 0, TOLG_MODE_SS = 1 };
enum { TOLG_E_ARG = -1, TOLG_E_WORKSPACE = -2, TOLG_E_LAUNCH = -3, TOLG_E_SINGULAR = -4 };
/* TOLG_ST_INTERNAL: a wavefront of the fused rollout gave up waiting for its producer (never expected; it
 * replaces a GPU hang by a visible status). */
enum { TOLG_ST_OK = 0, TOLG_ST_MAXREG = 1, TOLG_ST_NODESCENT = 2, TOLG_ST_NONFINITE = 3, TOLG_ST_INTERNAL = 4 };
/* tolg_options.schedule: how one accept-always MS iteration (line_search = 0, rollout = 'nonlinear') is
 * issued.  AUTO: the rollout and the re-linearisation of the new trajectory share one launch (k_rollout_lin);
 * SPLIT: separate rollout and linearisation launches (the only form for every other mode).  Same results
 * either way up to the summation order inside lin_knot (identical code). */
enum { TOLG_SCHED_AUTO = 0, TOLG_SCHED_SPLIT = 1 };

/* Problem = one (dynamics, cost) pair shared by the whole batch.
 * Replaces the constructor arguments of SE3Dynamics / RigidBodyDynamics / DroneDynamics
 * (traoptlibrary/traopt_dynamics.py:633-690, :906-970, :1214-1278) and of
 * SE3TrackingQuadraticGaussNewtonCost (traoptlibrary/traopt_cost.py:587-622). */
typedef struct {
  int32_t kind;   /* TOLG_DYN_* */
  int32_t m;      /* action size: 6 (SE3, RigidBody) or 4 (Drone) */
  int32_t N;      /* horizon */
  int32_t reserved;
  double dt;
  double J[36];   /* inertia diag(I_b, mass*I3); any SPD 6x6 is accepted */
  double Q[144];  /* stage weights, 12x12 (only the two 6x6 diagonal blocks are read, as in
                     traopt_cost.py:697,702) */
  double P[144];  /* terminal weights */
  double R[36];   /* m x m row-major */
  double pend_mass;   /* Pendulum3dDyanmics m      (traopt_dynamics.py:425; other kinds: ignored) */
  double pend_length; /* Pendulum3dDyanmics length (traopt_dynamics.py:425) */
} tolg_problem;

/* Replaces the keyword arguments of iLQR_Tracking_SE3_MS.__init__/fit and
 * iLQR_Tracking_SE3.__init__/fit (traoptlibrary/traopt_controller.py:2359-2363, :2443-2445,
 * :1837-1838, :1880-1881). */
typedef struct {
  int32_t mode;            /* TOLG_MODE_MS | TOLG_MODE_SS */
  int32_t max_iter;        /* n_iterations */
  int32_t line_search;     /* MS: merit-function search (:2549-2590); SS always backtracks */
  int32_t rollout_linear;  /* rollout == 'linear' (the reference constructors' default, :1837-1838, :2359-2363): on the device the
                              linear rollout is an affine recursion in the deviation, linear in the step size -- one sweep serves
                              every candidate of a line search (DESIGN.md section 4 "Linear rollouts") */
  double tol_grad;         /* tol_grad_norm */
  double tol_defect;       /* tol_d_norm (MS) */
  double max_reg;          /* max_reg (1e10) */
  int32_t schedule;        /* TOLG_SCHED_* (no reference counterpart: launch structure only) */
  int32_t check_every;     /* tolg_solve_batch: 0 = enqueue all max_iter iterations and never synchronise; k > 0 = issue
                              them k at a time and stop once every trajectory has finished (tolg_solve_iterate_until) */
} tolg_options;

typedef struct tolg_handle_s* tolg_handle_t;

/* Bytes of device workspace tolg_create needs for batches up to max_batch and max_iter
 * iterations. */
size_t tolg_workspace_bytes(const tolg_problem* prob, int32_t max_batch);

/* Build a solver instance on caller-provided device workspace.  d_q_ref [(N+1)][16],
 * d_xi_ref [(N+1)][6] are read once (the q_ref "manifisation" of traopt_cost.py:614).
 * The handle itself is a small host object; destroy frees only that. */
int tolg_create(const tolg_problem* prob, const double* d_q_ref, const double* d_xi_ref,
                int32_t max_batch, void* d_workspace, size_t workspace_bytes, void* stream,
                tolg_handle_t* out);
void tolg_destroy(tolg_handle_t h);

/* fit for a batch of B independent trajectories -- replaces B calls of
 * iLQR_Tracking_SE3_MS.fit (traoptlibrary/traopt_controller.py:2443-2639) or
 * iLQR_Tracking_SE3.fit (:1880-2013), i.e. the joblib fan-out of
 * visualization/perturb_all_compute.py:240-250.
 *   in : d_x0_q [B][16], d_x0_xi [B][6], d_us_init [B][N][m]
 *   out: d_xs_q [B][N+1][16], d_xs_xi [B][N+1][6], d_us [B][N][m]
 *        d_J_hist [B][max_iter]        cost after iteration k (what on_iteration appends)
 *        d_grad_hist [B][max_iter+1]   gradient norm evaluated in iteration k
 *        d_defect_hist [B][max_iter+1] MS: [0] initial defect, [k+1] after iteration k
 *        d_alpha_hist [B][max_iter], d_mu_hist [B][max_iter]
 *        d_iters [B] callbacks made, d_status [B] TOLG_ST_*, d_converged [B]
 * History buffers may be NULL.  Entries past d_iters[b] are left untouched. */
int tolg_solve_batch(tolg_handle_t h, const tolg_options* opt, int32_t B, const double* d_x0_q,
                     const double* d_x0_xi, const double* d_us_init, double* d_xs_q, double* d_xs_xi,
                     double* d_us, double* d_J_hist, double* d_grad_hist, double* d_defect_hist,
                     double* d_alpha_hist, double* d_mu_hist, int32_t* d_iters, int32_t* d_status,
                     int32_t* d_converged, void* stream);

/* The same solve split in three, so a caller (bench.py, a receding-horizon loop) can issue the
 * iterations in slices with the batch resident in HBM: begin = _initial_guess + first
 * _linearization (traopt_controller.py:2486-2507); iterate = n_iter passes of the loop body
 * (:2522-2626); end = unpack to the reference's 4x4 layout.  tolg_solve_batch == begin +
 * iterate(max_iter) + end. */
int tolg_solve_begin(tolg_handle_t h, const tolg_options* opt, int32_t B, const double* d_x0_q,
                     const double* d_x0_xi, const double* d_us_init, double* d_J_hist, double* d_grad_hist,
                     double* d_defect_hist, double* d_alpha_hist, double* d_mu_hist, void* stream);
/* tolg_solve_begin with a warm start of the shooting states: in MS mode knots 1..N of the initial guess are
 * d_xs_q_init [B][N+1][16] / d_xs_xi_init [B][N+1][6] (knot 0 is always x0; xs_init[b][0] is not read) in place of the
 * reference.  In SS mode the initial rollout decides the states as in tolg_solve_begin, and d_xs_*_init are ignored (may be
 * NULL).  Everything else -- the per-trajectory reference and weight rules, the held policy, the scalar reset, TOLG_E_ARG --
 * is tolg_solve_begin's; MS with either d_xs_*_init NULL is TOLG_E_ARG.  With xs_init = x0 followed by the reference knots
 * the solve is bitwise tolg_solve_begin's. */
int tolg_solve_begin_warm(tolg_handle_t h, const tolg_options* opt, int32_t B, const double* d_x0_q, const double* d_x0_xi,
                          const double* d_xs_q_init, const double* d_xs_xi_init, const double* d_us_init, double* d_J_hist,
                          double* d_grad_hist, double* d_defect_hist, double* d_alpha_hist, double* d_mu_hist, void* stream);
int tolg_solve_iterate(tolg_handle_t h, int32_t n_iter, void* stream);
int tolg_solve_end(tolg_handle_t h, double* d_xs_q, double* d_xs_xi, double* d_us, int32_t* d_iters,
                   int32_t* d_status, int32_t* d_converged, void* stream);
/* Up to n_iter iterations, issued check_every at a time; stops when no trajectory of the batch is iterating any more
 * -- the early exit of traopt_controller.py:2528-2532 (:1937-1942 single shooting) for the batch as a whole.  Unlike
 * every other entry point this one waits on the stream: after queueing slice s it waits for the count read back
 * behind slice s - 1, so the device never idles and a finished batch costs at most one more slice of launches
 * (finished trajectories are masked, their workgroups exit at once).  check_every = 0, or a solve nothing can end
 * (multiple shooting with tol_grad = 0 and no line search), is tolg_solve_iterate(n_iter).  *n_issued (may be NULL):
 * iterations queued. */
int tolg_solve_iterate_until(tolg_handle_t h, int32_t n_iter, int32_t check_every, int32_t* n_issued, void* stream);
/* Number of trajectories of the solve in flight that are still being iterated (not converged, not stopped by
 * a status), written to d_count[0] on `stream`.  Apart from tolg_solve_iterate_until the library never synchronises: with
 * check_every = 0 tolg_solve_batch enqueues max_iter iterations (finished trajectories are masked, finished workgroups
 * exit at once); a caller
 * that wants the early exit of traopt_controller.py:2528-2532 issues the iterations in slices and reads this
 * count between them, or calls tolg_solve_iterate_until, which pipelines exactly that. */
int tolg_solve_active_count(tolg_handle_t h, int32_t* d_count, void* stream);
/* Same export without ending the solve: what the per-iteration on_iteration callback of
 * traoptlibrary/traopt_controller.py:2621-2626 needs (current xs, us) when a caller wants it. */
int tolg_solve_peek(tolg_handle_t h, double* d_xs_q, double* d_xs_xi, double* d_us, int32_t* d_iters,
                    int32_t* d_status, int32_t* d_converged, void* stream);

/* Per-trajectory reference paths (no reference counterpart: the reference tracks one path per controller).
 * tolg_refs_bytes: bytes of the caller-owned buffer that holds the packed references of a batch of up to max_batch
 * trajectories, (N+1) * 13 * Bp * 8 with Bp = max_batch rounded up to a multiple of 4; 0 for an invalid problem.
 * tolg_set_refs: packs d_q_ref [B][N+1][16], d_xi_ref [B][N+1][6] (the layout of tolg_create) into d_refs on `stream`;
 * from then on every batch entry point of the handle -- tolg_solve_batch, tolg_solve_begin (the MS initial guess: knots
 * 1..N = trajectory b's own reference), iterate / iterate_until / peek / end, tolg_linearize_backward, tolg_rollout,
 * tolg_expected_change -- tracks trajectory b's reference, and must be called with this B (else TOLG_E_ARG).
 * tolg_al_update reads no reference; tolg_eval_knot keeps the reference of tolg_create.  Like tolg_set_al the buffer
 * stays caller-owned and is read by later calls.  d_q_ref = NULL returns the handle to the reference of tolg_create.
 * TOLG_E_ARG: B < 1 or B > max_batch, refs_bytes < tolg_refs_bytes(prob, B), a solve in flight (between
 * tolg_solve_begin and tolg_solve_end).
 *
 * tolg_set_ref_windows: the same packing, gathered from B longer paths d_path_q [B][T+1][16], d_path_xi [B][T+1][6]: knot i
 * of trajectory b's reference is knot min(t0[b] + t + i, T) of its path -- past the end the last knot is held, so any T >= 1
 * is accepted, T < N included.  d_t0 [B] (int32, on the device; NULL = 0) is each trajectory's phase on its path, t the
 * step.  Afterwards the handle is exactly as after tolg_set_refs with the windows (same buffer size, same B rules).
 * TOLG_E_ARG: those of tolg_set_refs, a NULL path, T < 1, t < 0.
 *
 * A receding-horizon (MPC) loop, every trajectory its own path and phase, with no host work per step:
 *   tolg_solve_begin + iterations + tolg_solve_end once from (x0, us_init) on window 0, then for each step t:
 *     tolg_mpc_advance(h, B, d_w_t, d_x_q, d_x_xi, d_u_t, d_xs_q_w, d_xs_xi_w, d_us_w, d_J_cl, stream);  apply u*_0, step
 *     tolg_set_ref_windows(h, B, d_path_q, d_path_xi, T, d_t0, t + 1, d_refs, refs_bytes, stream);
 *     tolg_solve_begin_warm(h, &opt, B, d_x_q, d_x_xi, d_xs_q_w, d_xs_xi_w, d_us_w, ...);     the shifted solution
 *     tolg_solve_iterate_until(h, n, opt.check_every, NULL, stream);       check_every = 0: a fixed count, no host read
 *     tolg_solve_end(h, d_xs_q, d_xs_xi, d_us, d_iters, d_status, d_converged, stream); */
size_t tolg_refs_bytes(const tolg_problem* prob, int32_t max_batch);
int tolg_set_refs(tolg_handle_t h, int32_t B, const double* d_q_ref, const double* d_xi_ref, void* d_refs, size_t refs_bytes,
                  void* stream);
int tolg_set_ref_windows(tolg_handle_t h, int32_t B, const double* d_path_q, const double* d_path_xi, int32_t T,
                         const int32_t* d_t0, int32_t t, void* d_refs, size_t refs_bytes, void* stream);

/* Per-trajectory cost weights (diagonal Q, P, R; the reference tunes one controller's weights by hand).
 * tolg_weights_bytes: bytes of the caller-owned buffer that holds the packed weights of a batch of up to max_batch
 * trajectories, (24 + m) * Bp * 8 with Bp = max_batch rounded up to a multiple of 4; 0 for an invalid problem.
 * tolg_set_weights: packs d_q_diag [B][12] (the diagonal of Q: rows 0..5 are the pose block W1, rows 6..11 the twist block
 * W2), d_p_diag [B][12] (the same for P) and d_r_diag [B][m] (the diagonal of R) into d_w on `stream`; from then on every
 * batch entry point of the handle -- tolg_solve_batch, tolg_solve_begin, iterate / iterate_until / peek / end,
 * tolg_linearize_backward, tolg_rollout, tolg_expected_change -- weights trajectory b's cost with its own diagonals, and
 * must be called with this B (else TOLG_E_ARG).  The weights are not read here: any value the caller gives is used (0 is
 * legal, a negative one makes the cost indefinite).  tolg_eval_knot keeps the weights of tolg_create.  Like tolg_set_refs
 * the buffer stays caller-owned and is read by later calls; d_q_diag = NULL returns the handle to the weights of
 * tolg_create.  Weights and references (tolg_set_refs) are set independently; when both are per trajectory they are for
 * the same B.
 * TOLG_E_ARG: B < 1 or B > max_batch, w_bytes < tolg_weights_bytes(prob, B), a solve in flight, references per
 * trajectory for another B. */
size_t tolg_weights_bytes(const tolg_problem* prob, int32_t max_batch);
int tolg_set_weights(tolg_handle_t h, int32_t B, const double* d_q_diag, const double* d_p_diag, const double* d_r_diag,
                     void* d_w, size_t w_bytes, void* stream);

/* Pose schedule: a factor s[b][i][k] >= 0 on entry k = 0..5 of the pose-weight diagonal (the first six diagonal entries of
 * Q / P: rotation error, then translation error) that knot i = 0..N of trajectory b reads -- gates or waypoints weighted
 * tightly at chosen knots, pose tracking switched off over a stretch.  Wherever a kernel reads that entry for knot i it uses
 * s[b][i][k] times it, whichever of Q and P the knot selects (the terminal knot's rules included): l, l_x, l_xx of the
 * linearisation, the cost of every rollout and line search, l_x and l_xx of tolg_policy_value.  Twist weights, R and the
 * augmented-Lagrangian terms are untouched: the backward sweeps keep them as per-lane constants for the whole horizon, and
 * the pose block reaches them through the knot records, so a pose schedule changes no sweep.
 * The schedule sits on top of held per-trajectory weights (tolg_set_weights) and nothing else: every entry point that
 * reads trajectory b's weights reads its schedule too; tolg_eval_knot keeps the weights of tolg_create.
 * tolg_pose_schedule_bytes: bytes of the caller-owned buffer that holds the packed factors, (N+1) * 6 * Bp * 8 with
 * Bp = max_batch rounded up to a multiple of 4; 0 for an invalid problem or max_batch < 1.
 * tolg_set_pose_schedule: packs d_scale [B][N+1][6] into d_packed on `stream`.  The factors are not read here (a negative
 * one makes the cost indefinite).  The buffer stays caller-owned and is read by later calls.  d_scale = NULL detaches the
 * schedule; so does tolg_set_weights with d_q_diag = NULL.
 * TOLG_E_ARG: a solve in flight; no per-trajectory weights held, or held for another B; B < 1 or B > max_batch;
 * bytes < tolg_pose_schedule_bytes(prob, B).
 * tolg_set_pose_schedule_windows: the same packing gathered from B longer schedules d_path_scale [B][T+1][6] by the rule
 * of tolg_set_ref_windows: knot i of trajectory b takes source knot min(t0[b] + t + i, T), d_t0 = NULL: 0.
 * TOLG_E_ARG: those above, a NULL path, T < 1, t < 0. */
size_t tolg_pose_schedule_bytes(const tolg_problem* prob, int32_t max_batch);
int tolg_set_pose_schedule(tolg_handle_t h, int32_t B, const double* d_scale, void* d_packed, size_t bytes, void* stream);
int tolg_set_pose_schedule_windows(tolg_handle_t h, int32_t B, const double* d_path_scale, int32_t T, const int32_t* d_t0,
                                   int32_t t, void* d_packed, size_t bytes, void* stream);

/* Augmented-Lagrangian box input constraint lb <= u <= ub -- replaces ALConstrainedCost wrapping the
 * tracking cost with an InputConstraint (traoptlibrary/traopt_cost.py:1173-1320,
 * traoptlibrary/traopt_constraints.py:66-169).  d_lb/d_ub [m]; d_lambda, d_imu [B][N][2m] (multipliers
 * and the diagonal of I_mu for g = [lb - u; u - ub]; the terminal knot has g = 0).  The buffers stay
 * caller-owned and are read by every later solve on this handle; d_lb = NULL switches AL off. */
int tolg_set_al(tolg_handle_t h, const double* d_lb, const double* d_ub, const double* d_lambda,
                const double* d_imu);

/* The input box per trajectory or per knot: tolg_set_al's constraint with bounds that differ over the batch (two vehicles
 * with different thrust limits, a sweep of a saturation level) or over the horizon as well (a derating that starts
 * mid-horizon, a box tightened by kappa sigma_u of tolg_policy_covariance's var_u).
 *   TOLG_BOX_PER_TRAJECTORY 1   d_lb, d_ub [B][m]
 *   TOLG_BOX_PER_KNOT       2   d_lb, d_ub [B][N][m]
 * The rows g = [lb - u_i; u_i - ub], i < N, the cost terms, the multipliers d_lambda, d_imu [B][N][2m] and the terminal knot
 * (g = 0) are tolg_set_al's; only where lb and ub of a row are read changes.  Nothing is packed: the bounds stay
 * caller-owned and are read in place by every later solve, entry a of knot i of trajectory b at b * stride_b + i * stride_i
 * + a with element strides (m, 0) or (N m, m), beside the multipliers.  The bounds must be finite (lambda * g with an
 * infinite g is NaN; a missing limit is a wide finite one) and are not read here.
 * It and tolg_set_al replace each other; d_lb = NULL detaches the box, whichever call attached it.  While attached, the
 * handle runs the kernels it runs with position slots attached, whether any are or not (those forms read the box strided;
 * with tolg_set_al's shared box they read it with strides 0), every batch entry point must be called with this B, and
 * tolg_eval_knot, which probes with the shared forms, is refused.  tolg_al_update_state, tolg_al_mpc_step and
 * tolg_al_mpc_step_pose read whichever box the handle holds; tolg_al_update takes the [m] box of its own arguments.  The held
 * policy is left alone: its gains belong to the problem that was solved.
 * TOLG_E_ARG, the handle unchanged: form outside 1..2; B < 1 or B > max_batch; a NULL d_ub, d_lambda or d_imu; a solve in
 * flight; another per-trajectory input held for another B; a model of the SO3 family or the pendulum (refused, they keep
 * the shared box: the per-trajectory forms are not offered for them); bounds of 4 GB or more (B m >= 2^29 for form 1, B N m >= 2^29 for form 2:
 * the kernels address them with 32-bit byte offsets).
 * Not offered: box bounds on the twist.  They would be state rows whose l_xx falls on the velocity block, which the knot
 * record does not carry and both backward sweeps rebuild from the weights.
 * tolg_set_al_box_windows: the boxes of step t of a receding-horizon loop gathered on `stream` from world-time paths
 * d_path_lb, d_path_ub [B][T+1][m] into the caller-owned d_lb_win, d_ub_win [B][N][m] by the rule of tolg_set_ref_windows:
 * knot i of trajectory b takes path knot min(t0[b] + t + i, T), d_t0 = NULL: 0; any T >= 1, T < N included.  It then leaves
 * the handle as tolg_set_al_box(h, B, TOLG_BOX_PER_KNOT, d_lb_win, d_ub_win, d_lambda, d_imu) would.
 * TOLG_E_ARG: those above, a NULL path or window buffer, T < 1, t < 0. */
#define TOLG_BOX_PER_TRAJECTORY 1
#define TOLG_BOX_PER_KNOT 2
int tolg_set_al_box(tolg_handle_t h, int32_t B, int32_t form, const double* d_lb, const double* d_ub, const double* d_lambda,
                    const double* d_imu);
int tolg_set_al_box_windows(tolg_handle_t h, int32_t B, const double* d_path_lb, const double* d_path_ub, int32_t T,
                            const int32_t* d_t0, int32_t t, double* d_lb_win, double* d_ub_win, const double* d_lambda,
                            const double* d_imu, void* stream);

/* One outer iteration of AL_iLQR_Tracking_SE3_MS (traoptlibrary/traopt_controller.py:3242-3250,
 * :3270-3290) for B independent problems on the controls d_us [B][N][m] of the inner solve:
 * d_maxviol[b] = max_k g_k over all knots; if it is below tol_constr the problem is marked in
 * d_al_converged[b] and left alone (now and in later calls); otherwise
 * lambda <- max(0, lambda + I_mu g), mu <- min(mu_scale*mu, mu_max),
 * I_mu <- (g < 0 and lambda_new == 0) ? 0 : mu_new. */
int tolg_al_update(tolg_handle_t h, int32_t B, const double* d_us, const double* d_lb, const double* d_ub,
                   double* d_lambda, double* d_imu, double* d_mu, double mu_scale, double mu_max,
                   double tol_constr, double* d_maxviol, int32_t* d_al_converged, void* stream);

/* Augmented-Lagrangian keep-out spheres, a state constraint (ALConstrainedCost wrapping the tracking cost with a
 * BaseConstraint, traoptlibrary/traopt_cost.py:1173-1320, traoptlibrary/traopt_constraints.py:5-63).  Trajectory b keeps out of
 * its own K spheres (c_k, r_k), 1 <= K <= TOLG_MAX_OBSTACLES, at every knot i = 0..N, terminal included:
 *   g_k(x_i) = r_k^2 - |t_i - c_k|^2 <= 0      (t_i: the translation of the pose X_i = (R_i, t_i))
 * In the error coordinates of l_x (right perturbation X Exp(delta), twist order [omega, v]: tolg_policy_rollout's dx0, d_lx of
 * tolg_linearize_backward) g_x = [0_3, -2 (t - c)^T R, 0_6], g_u = 0, and the cost gains the reference's Gauss-Newton terms
 *   l += lambda_ik g_k + I_ik g_k^2 / 2,  l_x[3:6] += g_x^T (lambda_ik + I_ik g_k),  l_xx[3:6,3:6] += I_ik g_x^T g_x.
 * TOLG_DYN_SE3, _RIGIDBODY and _DRONE (diagonal or dense inertia); the SO3 family has no translation.
 *
 * tolg_obstacles_bytes: bytes of the caller-owned buffer that holds the packed geometry of a batch of up to max_batch
 * trajectories with K spheres each, 4 K Bp 8 with Bp = max_batch rounded up to a multiple of 4; 0 for an invalid problem, a
 * kind of the SO3 family or K out of range.
 * tolg_set_al_obstacles: packs d_obs [B][K][4] = (cx, cy, cz, r) into d_packed on `stream` and attaches the multipliers
 * d_lambda [B][N+1][K] and the diagonal of I_mu d_imu [B][N+1][K]; like tolg_set_al these stay caller-owned and are read by
 * every later solve on the handle.  From then on every batch entry point -- tolg_solve_batch, tolg_solve_begin(_warm), iterate /
 * iterate_until / peek / end, tolg_linearize_backward, tolg_rollout, tolg_expected_change -- adds the terms of trajectory b's
 * spheres to its cost, and must be called with this B (else TOLG_E_ARG).  With tolg_set_al attached too the cost carries both
 * sets of terms.  tolg_eval_knot ignores them (as it ignores per-trajectory references and weights); tolg_policy_rollout and
 * tolg_mpc_advance report the tracking cost only.  d_obs = NULL detaches the spheres.  The held policy is left alone.
 * With tolg_set_al_obstacle_kinds (below) slot k is a keep-in sphere (|d|^2 - r^2), a half-space (n.t - o, fields nx ny nz o) or
 * a vertical column (r^2 - (dx^2 + dy^2)) instead, with clearances r - |d|, o - n.t and sqrt(dx^2 + dy^2) - r; this call, the
 * moving form and the window form keep the kinds when K is the K attached and reset them to keep-out spheres otherwise.
 * TOLG_E_ARG: B < 1 or B > max_batch, K out of range, a NULL multiplier or buffer, packed_bytes < tolg_obstacles_bytes(prob, B,
 * K), a solve in flight, references or weights per trajectory for another B, a kind of the SO3 family. */
#define TOLG_MAX_OBSTACLES 16
size_t tolg_obstacles_bytes(const tolg_problem* prob, int32_t max_batch, int32_t K);
int tolg_set_al_obstacles(tolg_handle_t h, int32_t B, int32_t K, const double* d_obs, const double* d_lambda,
                          const double* d_imu, void* d_packed, size_t packed_bytes, void* stream);

/* Position constraints beyond the keep-out sphere: every slot k of the K attached has a kind, the same for every trajectory and
 * every knot (batch-shared, so no wave diverges on it).  The four fields (f0, f1, f2, f3) of a slot stay where the three
 * tolg_set_al_obstacles* calls put them and are read per kind; with d = t - (f0, f1, f2):
 *   kind                   fields            row g <= 0              grad_t g          clearance (>= 0 inside the allowed set)
 *   TOLG_OBS_KEEP_OUT  0   cx cy cz r        r^2 - |d|^2             -2 d              |d| - r
 *   TOLG_OBS_KEEP_IN   1   cx cy cz r        |d|^2 - r^2              2 d              r - |d|             (a geofence)
 *   TOLG_OBS_HALF_SPACE 2  nx ny nz o        n.t - o                  n                o - n.t             (|n| = 1, as given)
 *   TOLG_OBS_COLUMN_Z  3   cx cy -  r        r^2 - (dx^2 + dy^2)     -2 (dx, dy, 0)    sqrt(dx^2 + dy^2) - r   (axis along world z)
 * Each depends on the position alone, so in the error coordinates g_x = [0_3, (grad_t g)^T R, 0_6]: the block the sphere fills,
 * and the cost terms are the sphere's with that g and g_x.  The half-space normal is not rescaled: o is measured along it.
 * tolg_set_al_obstacle_kinds: kinds [K] on the HOST, each one of TOLG_OBS_*; NULL makes every slot a keep-out sphere again.
 * Called after an attach (tolg_set_al_obstacles, _moving or _windows), for the K attached; stream-ordered like the attach.
 * Attaching again with the same K, in any of the three forms, keeps the kinds (an MPC loop attaches every step); attaching
 * with another K, or detaching, makes every slot TOLG_OBS_KEEP_OUT.  A handle on which it was never called runs keep-out
 * spheres.  The multiplier rule, the multiplier shape [B][N+1][K] and the packed layout are unchanged.  The held policy is
 * left alone.
 * TOLG_E_ARG: nothing attached, K other than the attached K, a kind outside 0..3, a solve in flight. */
#define TOLG_OBS_KEEP_OUT 0
#define TOLG_OBS_KEEP_IN 1
#define TOLG_OBS_HALF_SPACE 2
#define TOLG_OBS_COLUMN_Z 3
int tolg_set_al_obstacle_kinds(tolg_handle_t h, int32_t K, const int32_t* kinds, void* stream);

/* Keep-out spheres that move: the same constraint with its geometry given per knot, so that another vehicle's predicted path, a
 * sphere that exists around some knots only, or a radius inflated by the knot's position covariance (tolg_policy_covariance)
 * can be stated.  d_obs is [B][N+1][K][4] = (cx, cy, cz, r) of trajectory b at knot i, terminal knot included:
 *   g_k(x_i) = r_ik^2 - |t_i - c_ik|^2 <= 0
 * tolg_obstacles_moving_bytes: (N+1) 4 K Bp 8, the packed size ([N+1][4K][Bp]: field f = 4k + c of knot i of trajectory b at
 * (i 4K + f) Bp + b, padded trajectories replicate B-1); 0 under the rules of tolg_obstacles_bytes.
 * tolg_set_al_obstacles_moving: everything else is tolg_set_al_obstacles' -- the caller-owned multipliers [B][N+1][K], the batch
 * entry points that add the terms and demand this B, tolg_eval_knot / tolg_policy_* / tolg_mpc_advance ignoring them, the held
 * policy left alone, and its TOLG_E_ARG list with packed_bytes checked against tolg_obstacles_moving_bytes(prob, B, K).
 * Attaching either form replaces the other; d_obs = NULL in either call detaches.  tolg_al_update_state reads whichever form is
 * attached.  The kernels are those of the static form: the geometry address gains a knot stride, 0 there and 4 K Bp here.
 * Cost: 211 MB of packed geometry at 4096 x 200 with K = 8, and where the static form reads the same 4K values at every knot
 * (cached), this one streams 4K new values per knot and trajectory; see INTEGRATION.md 3k for what was measured. */
size_t tolg_obstacles_moving_bytes(const tolg_problem* prob, int32_t max_batch, int32_t K);
int tolg_set_al_obstacles_moving(tolg_handle_t h, int32_t B, int32_t K, const double* d_obs, const double* d_lambda,
                                 const double* d_imu, void* d_packed, size_t packed_bytes, void* stream);

/* Pose constraints: where the vehicle points.  A second slot family beside the position slots of tolg_set_al_obstacles* and
 * independent of them, with its own geometry, kinds and multipliers: trajectory b has K slots, 1 <= K <=
 * TOLG_MAX_POSE_CONSTRAINTS, of four fields each, g_k(R_i, t_i) <= 0 at every knot i = 0..N, terminal included.  The kind of
 * slot k is the same for every trajectory and every knot (batch-shared: no wave diverges on it).  The body axes are fixed: e3 =
 * (0, 0, 1) is the thrust axis of TOLG_DYN_DRONE, e1 = (1, 0, 0) is forward.  In the error coordinates of l_x (right
 * perturbation X Exp(delta), twist order [omega, v]) g_x = [g_omega, g_v, 0_6], g_u = 0:
 *   kind                    fields                     row g <= 0                        g_omega        g_v               margin (>= 0 inside)
 *   TOLG_POSE_TILT_CONE 0   nx ny nz c = cos(max tilt) c - n^T R e3                      (R^T n) x e3   0                 n^T R e3 - c
 *   TOLG_POSE_VIEW_CONE 1   px py pz c = cos(half angle) c |b| - e1^T b, b = R^T (p - t) b x e1         e1 - c b / |b|    e1^T b / |b| - c
 * n is a world axis of unit norm, used as given; p is a world target.  -1 < c < 1.  The cost gains the reference's Gauss-Newton
 * terms (ALConstrainedCost, no g_xx), as for the spheres:
 *   l += lambda_ik g_k + I_ik g_k^2 / 2,  l_x[0:6] += g_x (lambda_ik + I_ik g_k),  l_xx[0:6,0:6] += I_ik g_x g_x^T.
 * The knot record, both backward sweeps, the gains and the held policy are those of every other solve: the pose block of l_xx
 * is stored whole already.  Two degenerate points: the tilt gradient vanishes at the antipode of the axis (R e3 = -n, where g
 * is largest), so a solve started exactly there is not pushed out by this row; the view row is not differentiable at t = p
 * (b = 0: g_v divides by |b|), so the target must stay off the path.  Constraints on the twist are not offered: the twist
 * block of l_xx is a per-lane constant of the sweeps.
 *
 * tolg_pose_constraints_bytes: bytes of the caller-owned buffer that holds the packed geometry, 4 K Bp 8 with Bp = max_batch
 * rounded up to a multiple of 4, times N + 1 with per_knot; 0 for an invalid problem, a kind of the SO3 family or K out of range.
 * tolg_set_al_pose_constraints: kinds [K] on the HOST, each TOLG_POSE_*; packs d_geo [B][K][4], or with per_knot != 0
 * [B][N+1][K][4] (the geometry of every knot: a view target that moves, a tilt limit that tightens near a gate), into d_packed
 * on `stream` ([knots][4K][Bp], coalesced over the batch, padded trajectories replicate B-1) and attaches the multipliers
 * d_lambda [B][N+1][K] and the diagonal of I_mu d_imu [B][N+1][K], caller-owned and read by every later solve on the handle.
 * From then on every batch entry point that adds the terms of the position slots adds these too and must be called with this B;
 * the handle runs the kernels it runs with position slots attached, whether any are or not.  tolg_al_update_state evaluates
 * the pose rows on the poses it is handed and moves these multipliers under its one rule, the one mu per problem, the joint
 * d_maxviol and d_al_converged.  tolg_eval_knot, the covariance and the value sweep ignore the family, as they ignore the
 * spheres; the policy rollouts ignore it in J (the tracking cost alone) and report its margins where asked
 * (tolg_policy_rollout_margins, tolg_policy_rollout_estimated_limited).  tolg_al_mpc_step refuses while the family is attached; tolg_al_mpc_step_pose is the step that takes
 * the pose rows as its third row set and shifts these multipliers with the others.  d_geo = NULL detaches.  The held policy is
 * left alone.
 * TOLG_E_ARG: K outside 1..TOLG_MAX_POSE_CONSTRAINTS, a kind outside 0..1, NULL kinds, multipliers or buffer, B < 1 or B >
 * max_batch, packed_bytes below tolg_pose_constraints_bytes(prob, B, K, per_knot), a solve in flight, another per-trajectory
 * input held for another B, a kind of the SO3 family.  A refused call changes nothing. */
#define TOLG_MAX_POSE_CONSTRAINTS 8
#define TOLG_POSE_TILT_CONE 0
#define TOLG_POSE_VIEW_CONE 1
size_t tolg_pose_constraints_bytes(const tolg_problem* prob, int32_t max_batch, int32_t K, int32_t per_knot);
int tolg_set_al_pose_constraints(tolg_handle_t h, int32_t B, int32_t K, const int32_t* kinds, const double* d_geo,
                                 int32_t per_knot, const double* d_lambda, const double* d_imu, void* d_packed,
                                 size_t packed_bytes, void* stream);

/* tolg_set_al_pose_constraint_windows: the pose slots of step t gathered on the device from world-time paths, d_path_geo
 * [B][T+1][K][4] = the four fields of trajectory b's slots at world knot s (a view target that moves in world time): knot i of
 * the window takes world knot min(t0[b] + t + i, T) (tolg_set_ref_windows' rule, one index helper for every window form; d_t0
 * NULL: 0; any T >= 1, T < N included).  Afterwards the handle is exactly as after tolg_set_al_pose_constraints(..., per_knot
 * = 1, ...) with the gathered [B][N+1][K][4] array: the same packed bytes (tolg_pose_constraints_bytes(prob, B, K, 1)), the
 * same multipliers, the same rules for B.  A re-attach with the same K, an MPC loop's at every step, leaves the position
 * slots and the kernels the handle runs as they are.  d_path_geo = NULL detaches.  The held policy is left alone.
 * TOLG_E_ARG: those of tolg_set_al_pose_constraints, T < 1, t < 0. */
int tolg_set_al_pose_constraint_windows(tolg_handle_t h, int32_t B, int32_t K, const int32_t* kinds, const double* d_path_geo,
                                        int32_t T, const int32_t* d_t0, int32_t t, const double* d_lambda, const double* d_imu,
                                        void* d_packed, size_t packed_bytes, void* stream);

/* One outer iteration of AL_iLQR_Tracking_SE3_MS (traoptlibrary/traopt_controller.py:3242-3250, :3270-3290) over every
 * constraint attached to the handle: the input box of tolg_set_al on d_us [B][N][m] and the spheres of tolg_set_al_obstacles
 * on the positions of d_xs_q [B][N+1][16].  d_maxviol[b] = the largest g of them all (the box contributes its terminal rows
 * g = 0); below tol_constr the problem is marked in d_al_converged[b] and left alone, otherwise both multiplier sets (the
 * attached d_lambda / d_imu of either call) follow the rule of tolg_al_update with one mu per problem, d_mu[b].  d_us may be
 * NULL without a box, d_xs_q without spheres.  tolg_al_update is unchanged.  The row of slot k is the row of its kind
 * (tolg_set_al_obstacle_kinds: r^2 - |d|^2, |d|^2 - r^2, n.t - o or r^2 - (dx^2 + dy^2)); the rule is the same for all.
 * Pose slots (tolg_set_al_pose_constraints) are a third row set under the same rule: c - n^T R e3 or c |b| - e1^T b on the
 * whole pose of d_xs_q, with their own multipliers.
 * TOLG_E_ARG: nothing attached, B < 1 or B > max_batch, B other than the spheres' or the pose slots' batch, a NULL input the
 * attached constraints need. */
int tolg_al_update_state(tolg_handle_t h, int32_t B, const double* d_xs_q, const double* d_us, double* d_mu, double mu_scale,
                         double mu_max, double tol_constr, double* d_maxviol, int32_t* d_al_converged, void* stream);

/* Constrained receding-horizon MPC: the multipliers follow the window.  tolg_al_mpc_step is the outer update of one MPC step
 * over everything attached to the handle, without tolg_al_update_state's sticky d_al_converged -- in a closed loop every step is
 * a new problem -- followed, with shift == 1, by a one-knot shift of both multiplier sets, in place in the caller-owned buffers
 * the handle points at: the warm start of the duals, as tolg_mpc_advance's shift is that of the states and controls.
 * The rows g of trajectory b are tolg_al_update_state's: the box rows [lb - u_i; u_i - ub], i < N, and the sphere rows
 * r_ik^2 - |t_i - c_ik|^2, i <= N, of whichever geometry form is attached when the call runs (a slot of another kind: the row
 * of that kind, tolg_set_al_obstacle_kinds: |d|^2 - r^2, n.t - o or r^2 - (dx^2 + dy^2)).  Then
 *   mv = max g        (the box contributes its terminal zero rows: mv starts at 0 with a box, at -inf without; NaN is passed over)
 *   d_maxviol[b] = mv (d_maxviol may be NULL)
 *   mu_new = mv < tol_constr ? mu[b] : min(mu_scale mu[b], mu_max)
 *   every row, whatever mv is:  lambda' = max(0, lambda + I_mu g),  I_mu' = (g < 0 and lambda' == 0) ? 0 : mu_new
 *   d_mu[b] = mu_new
 * so a satisfied problem still lets its multipliers relax and only mu stops growing.  With shift == 1
 *   box multipliers    [B][N][2m]:  row i takes row' i+1, i = 0..N-2, row N-1 keeps row' N-1;
 *   sphere multipliers [B][N+1][K]: row i takes row' i+1, i = 0..N-1, row N keeps row' N
 * (the last knot held, as tolg_set_ref_windows and us_warm hold theirs).  d_us may be NULL without a box, d_xs_q without
 * spheres.  The held policy is left alone: tolg_mpc_advance behind this call gives the bits it gave before it.
 * tolg_al_update and tolg_al_update_state are unchanged.  One workgroup per trajectory; cost: INTEGRATION.md 3m.
 * TOLG_E_ARG: nothing attached, B < 1 or B > max_batch, B other than the spheres' batch, a NULL input the attached constraints
 * need, a NULL d_mu, shift other than 0 or 1, a solve in flight, pose constraints attached (tolg_set_al_pose_constraints). */
int tolg_al_mpc_step(tolg_handle_t h, int32_t B, const double* d_xs_q, const double* d_us, double* d_mu, double mu_scale,
                     double mu_max, double tol_constr, double* d_maxviol, int32_t shift, void* stream);

/* tolg_al_mpc_step_pose: tolg_al_mpc_step with the pose slots attached (tolg_set_al_pose_constraints, static or per knot, or
 * tolg_set_al_pose_constraint_windows) as a third row set -- the step of a loop whose planner holds attitude limits.
 * tolg_al_mpc_step itself keeps its contract and refuses while the family is attached; this call takes the same arguments and
 * adds the pose rows c - n^T R e3 or c |b| - e1^T b, i <= N, on the poses of d_xs_q: they join mv (which still starts at 0 with
 * a box and at -inf without), the one mu per problem and d_maxviol, their multipliers [B][N+1][Kp] follow the same rule, and
 * with shift == 1 they shift as the sphere multipliers do: row i takes row' i+1, i = 0..N-1, row N keeps row' N.  With no pose
 * family attached the call is tolg_al_mpc_step, bit for bit.  The held policy is left alone.
 * TOLG_E_ARG: those of tolg_al_mpc_step but the family's presence, and as tolg_al_update_state has them: a pose family attached
 * for another B, a NULL d_xs_q with one attached. */
int tolg_al_mpc_step_pose(tolg_handle_t h, int32_t B, const double* d_xs_q, const double* d_us, double* d_mu, double mu_scale,
                          double mu_max, double tol_constr, double* d_maxviol, int32_t shift, void* stream);

/* tolg_set_al_obstacle_windows: the moving spheres of step t gathered on the device from world-time paths, d_path_obs
 * [B][T+1][K][4] = (cx, cy, cz, r) of trajectory b's spheres at world knot s: knot i of the window takes world knot
 * min(t0[b] + t + i, T) (tolg_set_ref_windows' rule; d_t0 NULL: 0; any T >= 1, T < N included).  Afterwards the handle is
 * exactly as after tolg_set_al_obstacles_moving with the gathered [B][N+1][K][4] array: the same packed bytes
 * (tolg_obstacles_moving_bytes), the same multipliers, the same rules for B.  d_path_obs = NULL detaches.  The held policy is
 * left alone.
 * TOLG_E_ARG: those of tolg_set_al_obstacles_moving, T < 1, t < 0. */
int tolg_set_al_obstacle_windows(tolg_handle_t h, int32_t B, int32_t K, const double* d_path_obs, int32_t T,
                                 const int32_t* d_t0, int32_t t, const double* d_lambda, const double* d_imu, void* d_packed,
                                 size_t packed_bytes, void* stream);

/* One linearisation + backward pass on given trajectories (unit-parity entry point): replaces
 * iLQR_Tracking_SE3_MS._linearization + _backward_pass + _gradient_wrt_control
 * (traoptlibrary/traopt_controller.py:2823-3093; ms = 0: the SS variants :2098-2349).
 *   in : d_xs_q [B][N+1][16], d_xs_xi [B][N+1][6], d_us [B][N][m], mu/delta in d_mu_delta [B][2]
 *   out: d_Fx [B][N][12][12], d_d [B][N][12], d_lx [B][N+1][12], d_lxx11 [B][N+1][6][6],
 *        d_k [B][N][m], d_K [B][N][m][12], d_J [B], d_dnorm [B], d_grad [B],
 *        d_mu_delta updated.  Any output may be NULL. */
int tolg_linearize_backward(tolg_handle_t h, int32_t ms, double max_reg, int32_t B, const double* d_xs_q,
                            const double* d_xs_xi, const double* d_us, double* d_mu_delta, double* d_Fx,
                            double* d_d, double* d_lx, double* d_lxx11, double* d_k, double* d_K,
                            double* d_J, double* d_dnorm, double* d_grad, void* stream);

/* The reference's per-knot plugin methods for n states at knot i (i == N: terminal) -- replaces
 * dynamics.f / f_x / f_u (traoptlibrary/traopt_dynamics.py:789-850, :1403-1482) and cost.l / l_x / l_u /
 * l_xx / l_uu / _err (traoptlibrary/traopt_cost.py:659-867; with tolg_set_al active: ALConstrainedCost).
 *   in : d_x_q [n][16], d_x_xi [n][6], d_u [n][m] (ignored at the terminal knot)
 *   out: d_f_q [n][16], d_f_xi [n][6], d_Fx [n][12][12], d_Fu [n][12][m], d_l [n], d_lx [n][12],
 *        d_lxx [n][12][12], d_lu [n][m], d_luu [n][m][m], d_err [n][12] = [Log(x x_ref^-1); xi - xi_ref].
 * Any output may be NULL.  Uses the handle's workspace: not to be called during a solve in flight.  The cost terms are those of
 * the reference and weights of tolg_create, also on a handle with per-trajectory references (tolg_set_refs) or weights
 * (tolg_set_weights), and carry no keep-out sphere terms (tolg_set_al_obstacles). */
int tolg_eval_knot(tolg_handle_t h, int32_t i, int32_t n, const double* d_x_q, const double* d_x_xi,
                   const double* d_u, double* d_f_q, double* d_f_xi, double* d_Fx, double* d_Fu, double* d_l,
                   double* d_lx, double* d_lxx, double* d_lu, double* d_luu, double* d_err, void* stream);

/* One closed-loop rollout with the gains left by the last tolg_linearize_backward on the same
 * trajectories -- replaces iLQR_Tracking_SE3_MS._rollout (:2641-2740) / iLQR_Tracking_SE3._rollout
 * (:2030-2082).  out: d_xs_q_new, d_xs_xi_new, d_us_new (same shapes as the inputs). */
int tolg_rollout(tolg_handle_t h, int32_t ms, int32_t rollout_linear, double alpha, int32_t B,
                 double* d_xs_q_new, double* d_xs_xi_new, double* d_us_new, void* stream);

/* Unit-parity entry point for the merit search's preparation: the linear alpha = 1 rollout and
 * _expected_cost_change (traopt_controller.py:2550-2552, :2730-2737, :2756-2769) on the trajectory, records and
 * gains tolg_linearize_backward(ms = 1) left in the workspace.  form 0: the statement-by-statement kernel
 * (k_expected_change); 1: the ring form alone (k_expected_change_ring; d_flag[b] = 1 marks the trajectories it
 * hands back, whose d_ecc entries are NaN); 2: the ring form with the hand-back behind it -- what a solve runs.
 * out: d_ecc [B][2] (first-order, second-order term), d_flag [B] (may be NULL). */
int tolg_expected_change(tolg_handle_t h, int32_t form, int32_t B, double* d_ecc, int32_t* d_flag, void* stream);

/* The held policy: a nominal trajectory x*_i, u*_i and the time-varying feedback gains k_i, K_i about it, for one batch
 * of B trajectories -- what the reference's fit leaves in self._k / self._K (traoptlibrary/traopt_controller.py:2636-2637,
 * :2010-2011, :1322-1323, :692-693).  Two calls set it:
 *   - tolg_solve_end (and tolg_solve_batch through it): the final trajectory and the gains of the solve's last backward
 *     sweep.  For a trajectory that converged that sweep ran about its final trajectory; for one stopped by max_iter it ran
 *     about the iterate BEFORE the final one (the sweep of the last iteration produced the step to the final iterate);
 *   - tolg_linearize_backward: gains about exactly the trajectory it was given (the way to refresh the gains about the
 *     final iterate).
 * tolg_create, tolg_solve_begin and tolg_solve_begin_warm clear it; so does tolg_eval_knot (it overwrites the nominal
 * trajectory).  tolg_rollout (writes the candidate arrays only), tolg_expected_change, tolg_set_al, tolg_al_update,
 * tolg_set_refs, tolg_set_ref_windows, tolg_set_weights, tolg_set_al_obstacles, tolg_al_update_state, tolg_mpc_advance,
 * tolg_policy_covariance, tolg_policy_value, tolg_policy_rollout_limited, tolg_mpc_advance_limited,
 * tolg_policy_rollout_margins and tolg_policy_rollout_estimated_limited leave it; the calls that
 * read it use the
 * references and weights set when they run.
 * Both calls return TOLG_E_ARG when no policy is held, during a solve in flight, for a B other than the held batch's, when
 * references or weights per trajectory are set for another B, and (tolg_policy_rollout) for S < 1.  Neither modifies
 * the held policy: repeated calls give the same bits, and a later solve is unaffected.
 *
 * tolg_solve_gains: the gains in the coordinates of tolg_linearize_backward's d_k / d_K:
 *   out: d_k [B][N][m], d_K [B][N][m][12] (either may be NULL). */
int tolg_solve_gains(tolg_handle_t h, int32_t B, double* d_k, double* d_K, void* stream);

/* tolg_policy_rollout: S closed-loop rollouts per trajectory of the held policy -- the reference's _rollout with alpha = 0
 * and rollout = 'nonlinear' (traopt_controller.py:2030-2082) from a perturbed start.  Sample (b, s):
 *   x^_0 = x*_0 (+) dx0: pose q*_0 Exp(dx0[0:6]), twist xi*_0 + dx0[6:12] (the error coordinates of K: e_0 = dx0);
 *   i < N: e_i = [Log(q*_i^-1 q^_i); xi^_i - xi*_i], u^_i = u*_i + K_i e_i, x^_{i+1} = f(x^_i, u^_i) with the model's exact
 *          dynamics (whatever a solve's rollout option was), then xi^_{i+1} += w[b][s][i];
 *   J = sum_{i<N} l(x^_i, u^_i, i) + l_N(x^_N): the tracking cost, with trajectory b's own reference and weights when
 *       tolg_set_refs / tolg_set_weights are active; no augmented-Lagrangian terms (tolg_set_al does not change J).
 *   in : d_dx0 [B][S][12] or NULL (= 0), d_w [B][S][N][6] or NULL (= 0)
 *   out: d_J [B][S], d_status [B][S] (TOLG_ST_OK, or TOLG_ST_NONFINITE for a sample whose state, control or cost is not
 *        finite), d_xs_q [B][S][N+1][16], d_xs_xi [B][S][N+1][6], d_us [B][S][N][m]; every output may be NULL.
 * A sample's bits depend on neither S nor the other samples. */
int tolg_policy_rollout(tolg_handle_t h, int32_t B, int32_t S, const double* d_dx0, const double* d_w, double* d_J,
                        int32_t* d_status, double* d_xs_q, double* d_xs_xi, double* d_us, void* stream);

/* tolg_mpc_advance: one receding-horizon step on the held policy x*, u* (after tolg_solve_end):
 *   x_{t+1} = f(x*_0, u*_0) with the model's exact dynamics (whatever the solve's rollout option was), then xi_{t+1} += w[b]
 *   (the noise convention of tolg_policy_rollout); d_u_applied = u*_0;
 *   d_J_cl[b] += l(x*_0, u*_0): the stage cost at knot 0 of the current window, with trajectory b's reference and weights when
 *   set, no augmented-Lagrangian terms;
 *   the warm start of the next step in the caller layout, what tolg_solve_begin_warm reads: xs_warm[0] = x_{t+1},
 *   xs_warm[i] = x*_{i+1} (1 <= i < N), xs_warm[N] = f(x*_N, u*_{N-1}); us_warm[i] = u*_{i+1} (i < N-1), us_warm[N-1] = u*_{N-1}.
 *   in : d_w [B][6] or NULL (= 0)
 *   out: d_x_next_q [B][16], d_x_next_xi [B][6], d_u_applied [B][m], d_J_cl [B] (accumulated): each may be NULL;
 *        d_xs_q_warm [B][N+1][16], d_xs_xi_warm [B][N+1][6], d_us_warm [B][N][m]: required.
 * It does not modify the held policy (a second call gives the same bits) and returns TOLG_E_ARG under the conditions of
 * tolg_solve_gains, or for a NULL warm buffer. */
int tolg_mpc_advance(tolg_handle_t h, int32_t B, const double* d_w, double* d_x_next_q, double* d_x_next_xi,
                     double* d_u_applied, double* d_xs_q_warm, double* d_xs_xi_warm, double* d_us_warm, double* d_J_cl,
                     void* stream);

/* The two closed loops under an actuator box, and the clearance of the rollouts from the keep-out spheres the handle holds: the
 * check of the margins tolg_policy_covariance supplies to first order (a box tightened by the input variance the feedback
 * spends, radii inflated by the position covariance).  A real actuator clips, and a clipped loop is no longer the linear one
 * the covariance describes.  The box is an argument of each call and never held by the handle (tolg_set_al's box is the
 * planner's and is not read here).  Everything not named below is the rule of tolg_policy_rollout / tolg_mpc_advance: the sample
 * definition, the noise convention, references and weights per trajectory, the plant rules of tolg_set_plant, the status, NULL
 * outputs costing nothing, the TOLG_E_ARG conditions of tolg_solve_gains, the held policy left alone (repeated calls give the
 * same bits; a sample's bits depend on neither S nor the other samples).
 *
 * tolg_policy_rollout_limited: the commanded input is u~_i = u*_i + K_i e_i, the applied one
 *   u^_i[a] = u~ < lb ? lb : (u~ > ub ? ub : u~)   (not fmin / fmax: a NaN command stays NaN and TOLG_ST_NONFINITE shows it)
 * with trajectory b's box lb = d_u_lb[b], ub = d_u_ub[b].  u^_i is what the dynamics step on, what the stage cost is evaluated
 * at and what d_us holds.  -inf / +inf mean no limit on that input; the library does not read the box on the host, lb <= ub
 * is the caller's promise; for the SO3 family the box rows 3..5 must contain 0 (those inputs are zero).  J stays the tracking
 * cost alone.
 *   in : d_dx0, d_w as tolg_policy_rollout; d_u_lb, d_u_ub [B][m] each, or both NULL: no clamp, the call is then the clearance
 *        report alone
 *   out: d_J, d_status, d_xs_q, d_xs_xi, d_us as tolg_policy_rollout;
 *        d_n_sat [B][S]       the number of pairs (i, a) with u^ != u~ (a command outside the box; a NaN command is not one)
 *        d_u_excess [B][S]    max_{i,a} max(lb - u~, u~ - ub, 0): the margin the box would have needed (0 inside it; NaN
 *                             distances are passed over)
 *        d_clear [B][S]       min_{i = 0..N, k < K} (|t^_i - c_ik| - r_ik) over the spheres attached to the handle, the static
 *                             form with one geometry for every knot, the moving form with knot i's own; negative: penetration
 *                             (+inf if no distance is a number).  A slot of another kind (tolg_set_al_obstacle_kinds)
 *                             enters with the clearance of its kind: r - |d| (keep-in), o - n.t (half-space),
 *                             sqrt(dx^2 + dy^2) - r (column); negative: outside the allowed set
 *        d_clear_knot [B][S]  the first knot that attains the minimum (strict <, knots ascending, spheres ascending)
 *        every output may be NULL.
 * TOLG_E_ARG: the conditions of tolg_policy_rollout; exactly one NULL bound; a non-NULL d_clear or d_clear_knot with no spheres
 * attached (spheres attached for another B refuse every batch call, this one included).
 * Cost on an MI355X: see INTEGRATION.md 3l (the clamp is 2 m compare-selects per knot on a chain of over a microsecond per
 * knot; the clearance adds 4 K loads and a square root per knot).
 *
 * tolg_mpc_advance_limited: tolg_mpc_advance with the plant's input clipped: d_u_applied = clamp(u*_0) by trajectory b's box;
 * x_next and xs_warm[0] step with it, on the plant row where one is set; d_J_cl[b] += l(x*_0, u_applied); d_n_sat[b] (may be
 * NULL) counts the inputs of this step the box moved.  The warm tail xs_warm[N] and us_warm are tolg_mpc_advance's: the model
 * and the unclamped shift (the planner stays unconstrained, only the plant clips).
 * TOLG_E_ARG: the conditions of tolg_mpc_advance; a NULL bound (tolg_mpc_advance is the unclamped form). */
int tolg_policy_rollout_limited(tolg_handle_t h, int32_t B, int32_t S, const double* d_dx0, const double* d_w,
                                const double* d_u_lb, const double* d_u_ub, double* d_J, int32_t* d_status, double* d_xs_q,
                                double* d_xs_xi, double* d_us, int32_t* d_n_sat, double* d_u_excess, double* d_clear,
                                int32_t* d_clear_knot, void* stream);
int tolg_mpc_advance_limited(tolg_handle_t h, int32_t B, const double* d_w, const double* d_u_lb, const double* d_u_ub,
                             double* d_x_next_q, double* d_x_next_xi, double* d_u_applied, double* d_xs_q_warm,
                             double* d_xs_xi_warm, double* d_us_warm, double* d_J_cl, int32_t* d_n_sat, void* stream);

/* tolg_policy_rollout_margins: tolg_policy_rollout_limited with the sampled check of the attitude margin
 * (tighten_pose_constraints in the binding: kappa standard deviations on the cones' cosines) and, per knot, how many samples
 * left a family's allowed set.  Everything tolg_policy_rollout_limited states holds: the sample definition, the clamp, the
 * plant, references and weights per trajectory, the sample orders, J the tracking cost alone.  Four more outputs:
 *        d_pose_margin [B][S]  min_{i = 0..N, k < K} of the margin of pose slot k (the table at tolg_set_al_pose_constraints:
 *                              tilt cone n^T R e3 - c, view cone e1^T b / |b| - c with b = R^T (p - t)) at the sample's state
 *                              at knot i -- the state each step starts from, and the terminal one -- over the slots attached to
 *                              the handle: the static form, the per-knot form with knot i's own geometry, the window form as
 *                              gathered; negative: outside a cone (+inf if no margin is a number: a NaN margin, a view target
 *                              at the sample's position, is passed over)
 *        d_pose_knot [B][S]    the first knot that attains it (strict <, knots ascending, slots ascending)
 *        d_viol_pos [B][N+1]   the number of samples s whose clearance at knot i -- min over the position slots of the
 *                              clearance of the slot's kind, d_clear's terms -- is < 0
 *        d_viol_pose [B][N+1]  the same for the pose margins
 *        every output may be NULL.  A NaN is not a violation.  The library zeroes the two count arrays on `stream` ahead of the
 *        launch and the kernel adds to them with integer atomics: the counts do not depend on the order of the samples and are
 *        the same bits on every call.  A kappa-sigma margin promises a violation probability at EACH knot (Phi(-kappa) to
 *        first order, for Gaussian deviations): d_viol_*[b][i] / S is its estimate there, which a minimum over the horizon
 *        cannot give, and it shows where along the path a margin is thin.
 * With the four NULL the call is tolg_policy_rollout_limited, bit for bit.  Every output's bits are independent of which other
 * outputs are asked for.
 * TOLG_E_ARG: the conditions of tolg_policy_rollout_limited; a non-NULL d_pose_margin, d_pose_knot or d_viol_pose with no pose
 * family attached; a non-NULL d_viol_pos with no position slots attached (a family attached for another B refuses every batch
 * call; the SO3 family can attach neither).  A refused call changes nothing.
 * Cost on an MI355X: INTEGRATION.md 3s. */
int tolg_policy_rollout_margins(tolg_handle_t h, int32_t B, int32_t S, const double* d_dx0, const double* d_w,
                                const double* d_u_lb, const double* d_u_ub, double* d_J, int32_t* d_status, double* d_xs_q,
                                double* d_xs_xi, double* d_us, int32_t* d_n_sat, double* d_u_excess, double* d_clear,
                                int32_t* d_clear_knot, double* d_pose_margin, int32_t* d_pose_knot, int32_t* d_viol_pos,
                                int32_t* d_viol_pose, void* stream);

/* The two closed loops behind an actuator model: the input the dynamics step on is no longer the input the policy commanded at
 * that knot.  A motor or a reaction wheel has a first-order lag of one to three knots at the dt the workloads use, a slew limit
 * and a transport or computation delay of a whole knot or more, and that decides whether time-varying LQR gains survive on a
 * vehicle.  The model, per trajectory b and input a, at every knot i < N of a sample:
 *   c_i  = u*_i + K_i e_i                              the command (what the policy asks for)
 *   d_i  = c_{i-D}  for i >= D,  u_init  otherwise     transport delay of D = delay knots, one value for the whole call
 *   s_i  = d_i < lb ? lb : (d_i > ub ? ub : d_i)       the box, tolg_policy_rollout_limited's select (a NaN stays NaN)
 *   l_i  = s_i - beta * (s_i - a_{i-1})                lag, beta = exp(-dt / tau) in [0, 1), beta = 0: none
 *   dl   = l_i - a_{i-1}
 *   a_i  = dl > du ? a_{i-1} + du : (dl < -du ? a_{i-1} - du : l_i)    rate limit, du = du_max > 0 per knot, +inf: none
 *   a_{-1} = u_init = d_u_init[b], or u*_0 of trajectory b when d_u_init is NULL
 *   x_{i+1} = f(x_i, a_i) (+ noise)                    on the plant row where a plant is set
 * The stage cost and d_us take a_i.  Written this way beta = 0 gives l_i = s_i and du = +inf selects l_i, exactly: with d_beta
 * NULL or 0, d_du_max NULL or +inf and delay = 0 the rollout returns the bits of tolg_policy_rollout_margins for every output
 * they share.  lb, ub, beta, du_max and u_init are [B][m]; the library does not read them on the host (beta in [0, 1), du_max
 * > 0 and lb <= ub are the caller's promise; check_actuator in the binding converts tau and a rate and checks them).  For the
 * SO3 family rows 3..5 of lb, ub and u_init must contain or equal 0, the box's rule. */
#define TOLG_MAX_ACT_DELAY 4
typedef struct tolg_actuator {
  const double *d_lb, *d_ub;   /* [B][m], both or neither */
  const double *d_beta;        /* [B][m] or NULL (= 0) */
  const double *d_du_max;      /* [B][m] or NULL (= +inf) */
  const double *d_u_init;      /* [B][m] or NULL (= u*_0); unused by the MPC call */
  int32_t delay;               /* 0..TOLG_MAX_ACT_DELAY */
} tolg_actuator;
/* tolg_policy_rollout_actuated: tolg_policy_rollout_margins with the model above in place of the box alone.  Every rule of the
 * margins call not named here holds: plant, references and weights per trajectory, both sample orders, clearance and pose
 * outputs with their attach conditions, J the tracking cost alone, the held policy left alone, a sample's bits independent of S
 * and of its neighbours, an output's bits independent of which others are asked for.  d_n_sat and d_u_excess keep their
 * definitions, on the delayed command d_i.  Three more outputs, each may be NULL:
 *        d_u_cmd [B][S][N][m]  the commands c_i
 *        d_n_rate [B][S]       the number of pairs (i, a) the rate limit moved
 *        d_u_gap [B][S]        max_{i,a} |a_i - c_i| (fmax: a NaN is passed over), the distance between what was asked for and
 *                              what the vehicle got
 * TOLG_E_ARG: the margins call's conditions; act NULL; exactly one NULL bound; delay outside 0..TOLG_MAX_ACT_DELAY.  A refused
 * call changes nothing.
 * Cost on an MI355X: INTEGRATION.md 3t (measured at 4096 x 200, S = 16, over the margins call with the same box and
 * outputs: +20 % with delay = 0, +28 % with delay = 1, +33 % with delay = 4; the expectation of a few per cent did not hold).
 *
 * tolg_mpc_advance_actuated: tolg_mpc_advance_limited with the model on the single command c = u*_0 of the step.  The
 * actuator's memory between steps is the caller's d_act_state [B][1 + delay][m], updated in place: row 0 the last applied
 * input, rows 1..delay the pending commands, oldest first.  The row-1 command is applied at this step (delay = 0: c itself),
 * rows 2.. move down one row and c goes to row delay.  d_u_applied, x_next, xs_warm[0] and d_J_cl take the applied input; the
 * warm tail and us_warm are tolg_mpc_advance's (the planner does not know the actuator, as it does not know the box).
 * d_n_sat [B], d_n_rate [B]: the inputs of this step the box / the rate limit moved; each may be NULL.  A second call with a
 * restored d_act_state gives the same bits.
 * TOLG_E_ARG: the conditions of tolg_mpc_advance; a NULL d_act_state; act NULL, exactly one NULL bound, delay out of range.
 *
 * Out of scope: the output-feedback loop (tolg_policy_rollout_estimated carries two chains in one quad and has no registers
 * left for the actuator's state); an analytic companion in tolg_policy_covariance (the augmented state has 12 + m coordinates,
 * the sweep's layout is one 16-lane row per trajectory); an actuator model inside the planner. */
int tolg_policy_rollout_actuated(tolg_handle_t h, int32_t B, int32_t S, const double* d_dx0, const double* d_w,
                                 const tolg_actuator* act, double* d_J, int32_t* d_status, double* d_xs_q, double* d_xs_xi,
                                 double* d_us, int32_t* d_n_sat, double* d_u_excess, double* d_clear, int32_t* d_clear_knot,
                                 double* d_pose_margin, int32_t* d_pose_knot, int32_t* d_viol_pos, int32_t* d_viol_pose,
                                 double* d_u_cmd, int32_t* d_n_rate, double* d_u_gap, void* stream);
int tolg_mpc_advance_actuated(tolg_handle_t h, int32_t B, const double* d_w, const tolg_actuator* act, double* d_act_state,
                              double* d_x_next_q, double* d_x_next_xi, double* d_u_applied, double* d_xs_q_warm,
                              double* d_xs_xi_warm, double* d_us_warm, double* d_J_cl, int32_t* d_n_sat, int32_t* d_n_rate,
                              void* stream);

/* tolg_policy_covariance: the closed-loop covariance of the held policy to first order ("LinCov"), the analytic companion of
 * tolg_policy_rollout's sampling.  In the coordinates of tolg_policy_rollout and of K, e_i = [Log(q*_i^-1 q^_i); xi^_i - xi*_i]
 * (twist order [omega, v]), about the held nominal x*_i, u*_i:
 *   A_i = f_x(x*_i, u*_i), B_i = f_u(x*_i, u*_i)   the model's Jacobians, as tolg_eval_knot returns them, linearised by this
 *                                                  call at the held nominal states (the workspace's knot records are not
 *                                                  trusted: after a solve stopped by max_iter they belong to another iterate
 *                                                  than the gains, see above);
 *   Acl_i = A_i + B_i K_i
 *   Sigma_{i+1} = Acl_i Sigma_i Acl_i^T + E W E^T,  E = [0; I6],  i = 0 .. N-1
 * with Sigma_0 the covariance of the start error dx0 (12 x 12, PSD) and W the covariance of the twist disturbance w added after
 * every step (6 x 6, PSD).  This is a covariance, not a mean: multiple-shooting defects of the nominal are ignored.  The loop is
 * the linear, unsaturated one of the model: a plant (tolg_set_plant), an input box (tolg_set_al) and keep-out spheres
 * (tolg_set_al_obstacles) are ignored -- the same bits with and without them.
 *   in : d_Sigma0 [B][12][12] or NULL (= 0), d_W [B][6][6] or NULL (= 0); only the upper triangles are read
 *   out: d_Sigma [B][N+1][12][12]   computed as a symmetric matrix and mirrored: equal to its transpose to the bit
 *        d_var_x [B][N+1][12]       diag Sigma_i (the bits of d_Sigma's diagonal)
 *        d_var_u [B][N][m]          diag K_i Sigma_i K_i^T: the input variance the feedback spends
 *        d_pos_cov [B][N+1][6]      R*_i Sigma_i[3:6,3:6] R*_i^T, the position covariance in the world frame: xx xy xz yy yz zz
 * Every output may be NULL, and a NULL output costs nothing (d_Sigma is 0.95 GB at 4096 x 200).  Sigma0 = W = 0 gives exact zeros;
 * a trajectory's bits depend on neither B nor its neighbours, nor on which outputs are asked for.  For the SO3 family the state is
 * carried in the SE(3) layout as everywhere in this header: rows / columns 3..5 and 9..11 are the unused translation and linear
 * velocity (inputs 3..5 are zero and K's rows for them with it; pass zeros there, as tolg_policy_rollout's dx0 and w do).
 * The call does not modify the held policy.  TOLG_E_ARG: the conditions of tolg_solve_gains; a non-NULL d_pos_cov for a kind of
 * the SO3 family (no translation: the rule of tolg_set_al_obstacles). */
int tolg_policy_covariance(tolg_handle_t h, int32_t B, const double* d_Sigma0, const double* d_W, double* d_Sigma, double* d_var_x,
                           double* d_var_u, double* d_pos_cov, void* stream);

/* tolg_policy_value: the cost-to-go of the held policy, V_i(e) ~ p_i . e + e^T P_i e / 2, the backward companion of
 * tolg_policy_covariance.  In the same coordinates, e_i = [Log(q*_i^-1 q^_i); xi^_i - xi*_i] (twist order [omega, v]), about
 * the held nominal x*_i, u*_i:
 *   A_i, B_i, Acl_i = A_i + B_i K_i        as in tolg_policy_covariance: linearised by this call at the held nominal
 *   l_x, l_xx, l_u, l_uu at (x*_i, u*_i)   the tracking cost's derivatives as tolg_eval_knot gives them (Gauss-Newton l_xx,
 *                                          l_ux = 0), with trajectory b's own reference and weights when tolg_set_refs /
 *                                          tolg_set_weights are active; no augmented-Lagrangian or keep-out terms (the rule
 *                                          of tolg_policy_rollout's J)
 *   M_i = l_xx + K_i^T l_uu K_i  (i < N),  M_N = l_xx^N
 *   P_N = M_N,  p_N = l_x^N
 *   P_i = M_i + Acl_i^T P_{i+1} Acl_i,  p_i = l_x + K_i^T l_u + Acl_i^T p_{i+1}      i = N-1 .. 0
 *   price_i = tr(P_{i+1}[6:12,6:12] W) / 2      what the twist disturbance added after step i costs, i = 0 .. N-1
 *   excess  = tr(P_0 Sigma0) / 2 + sum_i price_i   the expected closed-loop cost above the unperturbed one under (Sigma0, W),
 *                                                  to second order in the model's linearisation
 * p_0 is the gradient of the closed-loop cost with respect to the start error dx0, and excess equals
 * sum_{i <= N} tr(M_i Sigma_i) / 2 with tolg_policy_covariance's Sigma_i (an exact identity of the two recursions).
 * This is the cost-to-go of the MODEL THE SOLVER PLANS WITH: the reference's Jacobians (its f_x and the Jacobian of its
 * tracking error are approximate) and Gauss-Newton Hessians, not exact derivatives.  Measured on the CPU restatement
 * (se3_tracking, N = 20) against central differences of the closed-loop cost: p_N[6:12] agrees to 2e-11 (the terminal cost is
 * quadratic in the twist), p_0 to 1.5e-3 of max |p_0| on an off-nominal policy and 6e-5 on a converged one, interior knots
 * to ~1e-4 -- a gap that does not shrink with the step of the difference; v^T P_0 v is within 1.3 % of the second difference.
 * Multiple-shooting defects of the nominal are ignored, as in the covariance; a plant, an input box and keep-out spheres
 * too -- the same bits with and without them.
 *   in : d_Sigma0 [B][12][12] or NULL (= 0), d_W [B][6][6] or NULL (= 0); only the upper triangles are read
 *   out: d_P [B][N+1][12][12]     computed as a symmetric matrix and mirrored: equal to its transpose to the bit
 *        d_p [B][N+1][12]
 *        d_diag_P [B][N+1][12]    diag P_i (the bits of d_P's diagonal)
 *        d_price [B][N]
 *        d_excess [B]
 * Every output may be NULL, and a NULL output costs nothing (d_P is 0.95 GB at 4096 x 200).  Sigma0 = W = 0, or both NULL,
 * gives exact zeros in d_price and d_excess; P and p do not depend on Sigma0 or W.  A trajectory's bits depend on neither B
 * nor its neighbours, nor on which outputs are asked for.  For the SO3 family the state is carried in the SE(3) layout as
 * everywhere in this header: rows / columns 3..5 and 9..11 (the unused translation and linear velocity) carry no cost --
 * they hold exact zeros when the weights and the gains' columns of those coordinates are zero, as they are for the embedded
 * problems; pass zeros there in Sigma0 and W.
 * The call does not modify the held policy.  TOLG_E_ARG: the conditions of tolg_solve_gains. */
int tolg_policy_value(tolg_handle_t h, int32_t B, const double* d_Sigma0, const double* d_W, double* d_P, double* d_p,
                      double* d_diag_P, double* d_price, double* d_excess, void* stream);

/* Output feedback: the held policy acting on a Kalman filter's estimate instead of the true state.  Every closed loop above
 * feeds the true state into u = u*_i + K_i e_i; a vehicle knows its state through noisy sensors only, and the covariance of
 * tolg_policy_covariance (and the margins derived from its d_pos_cov) is optimistic by what the estimate adds.  The two calls
 * below are the analytic recursion and its sampled check, in the error coordinates of K and of tolg_policy_rollout:
 * e = [Log(q*^-1 q); xi - xi*], twist order [omega, v], right perturbation x (+) d = (q Exp(d[0:6]), xi + d[6:12]).
 *
 * The measurement model, shared by both: coordinates of the error state, measured at every knot 0..N.
 *   mask      int32, 12 bits: bit j set = coordinate j is measured.  A host argument shared by the batch (as
 *             tolg_set_al_obstacle_kinds' kinds word); 0 is legal (no sensor).  SO3 family: bits 3..5 and 9..11 must be clear.
 *   d_V       [B][12] measurement-noise variances (diagonal noise covariance), > 0 and finite on the measured coordinates by
 *             the caller's promise; entries of unmeasured coordinates are not read; may be NULL when mask == 0.
 *
 * tolg_policy_covariance_estimated: one forward sweep.  A_i, B_i, Acl_i = A_i + B_i K_i are linearised by this call at the held
 * nominal exactly as tolg_policy_covariance does.  P is the covariance of the estimation error e - e^, S^ that of the estimate's
 * deviation e^; the filter's prior at knot 0 is the nominal: P_0^- = Sigma0, S^_0^- = 0.
 *   at knot i = 0..N:
 *     Sigma_i = S^_i^- + P_i^-                                             the true state's covariance
 *     P^+ = P_i^-; for each measured j ascending: s = P^+[j][j] + V[j], c = P^+[:, j], P^+ -= c c^T / s
 *     L_i[:, j] = P^+[:, j] / V[j] (measured j), 0 (unmeasured j)          the Kalman gain, no matrix inverse
 *     S^_i^+ = S^_i^- + (P_i^- - P^+)
 *   for i < N:
 *     var_u_i = diag K_i S^_i^+ K_i^T
 *     P_{i+1}^- = A_i P^+ A_i^T + E W E^T,  E = [0; I6];    S^_{i+1}^- = Acl_i S^_i^+ Acl_i^T
 * (sequential scalar updates are exact for a diagonal V; Sigma = S^ + P rests on the orthogonality of estimate and error.)
 * The recursion is first order in the MODEL's Jacobians, the ones the solver plans with (the note at tolg_policy_value): the
 * reference's f_x is approximate in its twist columns, by an amount that grows with the nominal twist (against central
 * differences of f: 4e-3 at |xi| = 0.1, 0.4 at |xi| = 3).  Perfect-state feedback suppresses what that leaves; a filter without
 * a twist sensor carries the twist's estimation error open loop through those columns, and on a fast nominal the sampled
 * loop below can differ from this recursion by far more than its sampling error.  Check with tolg_policy_rollout_estimated.
 *   in : d_Sigma0, d_W as tolg_policy_covariance (NULL = 0, upper triangles only); mask, d_V above
 *   out: d_Sigma [B][N+1][12][12]    the true state's covariance, equal to its transpose to the bit
 *        d_P_post [B][N+1][12][12]   P^+_i, equal to its transpose to the bit
 *        d_L [B][N+1][12][12]        the Kalman gains (what tolg_policy_rollout_estimated takes)
 *        d_var_x [B][N+1][12]        diag Sigma_i (the bits of d_Sigma's diagonal)
 *        d_var_est [B][N+1][12]      diag P^+_i (the bits of d_P_post's diagonal)
 *        d_var_u [B][N][m]           the input variance the feedback spends
 *        d_pos_cov [B][N+1][6]       as tolg_policy_covariance, from Sigma
 * Every output may be NULL, and a NULL output costs nothing.  A trajectory's bits depend on neither B nor its neighbours, nor on
 * which outputs are asked for.  Sigma0 = W = 0 gives exact zeros; mask = 0 gives L = 0, var_u = 0 and P_post = the prior.  A plant,
 * an input box and constraint geometry are ignored; the held policy is left alone.
 * TOLG_E_ARG: the conditions of tolg_solve_gains; a mask outside 12 bits; SO3-family bits 3..5 / 9..11; a NULL d_V with
 * mask != 0; a non-NULL d_pos_cov for the SO3 family.
 *
 * tolg_policy_rollout_estimated: S samples per trajectory of the nonlinear loop with a filter of scheduled gains.  Sample (b, s):
 *   x_0 = x*_0 (+) dx0,  x^_0 = x*_0
 *   at knot i = 0..N:
 *     y = x_i (+) n[b][s][i]
 *     r[j] = ([Log(q^^-1 q_y); xi_y - xi^])[j] for measured j, 0 otherwise
 *     x^ <- x^ (+) L_i r
 *   for i < N:
 *     e^ = [Log(q*_i^-1 q^); xi^ - xi*_i],  u = u*_i + K_i e^
 *     x_{i+1} = f(x_i, u), then xi += w[b][s][i];   x^_{i+1} = f(x^, u)         both on the model's exact dynamics
 * J is the tracking cost of the TRUE trajectory and the applied u, under the rules of tolg_policy_rollout.
 *   in : d_L [B][N+1][12][12] required: the call above's d_L or the caller's own (columns of unmeasured coordinates are not read);
 *        d_dx0 [B][S][12], d_w [B][S][N][6] as tolg_policy_rollout; d_n [B][S][N+1][12] measurement noise; each NULL = 0
 *   out: d_J, d_status, d_xs_q, d_xs_xi, d_us as tolg_policy_rollout (the true trajectory);
 *        d_est_q [B][S][N+1][16], d_est_xi [B][S][N+1][6]   the posterior estimates x^_i
 *        every output may be NULL.
 * A sample's bits depend on neither S nor the other samples; the held policy is left alone.  This call steps both chains with
 * the MODEL: an attached plant (tolg_set_plant) is ignored, as by every entry point outside the two rollouts, and the call
 * takes no input box (the call below does).
 * TOLG_E_ARG: the conditions of tolg_policy_rollout; a bad mask (above); a NULL d_L.
 *
 * tolg_policy_rollout_estimated_limited: the same loop under an actuator box and with the reports of
 * tolg_policy_rollout_margins -- what a clipped actuator does to a vehicle that sees through sensors, and whether a sample
 * hit anything.  The input u = u*_i + K_i e^ is clamped by tolg_policy_rollout_limited's three-way select to trajectory b's
 * box; BOTH chains step with the clamped input (the filter knows what the actuator did), and the cost and d_us take it.
 *   in : as above, then d_u_lb, d_u_ub [B][m], both or neither
 *   out: as above, then d_n_sat, d_u_excess, d_clear, d_clear_knot [B][S] as tolg_policy_rollout_limited and d_pose_margin,
 *        d_pose_knot [B][S], d_viol_pos, d_viol_pose [B][N+1] as tolg_policy_rollout_margins, all of them evaluated on the TRUE
 *        state x_i, never on the estimate; every output may be NULL.
 * With both bounds and every new output NULL the call is tolg_policy_rollout_estimated, bit for bit; every output's bits are
 * independent of which others are asked for.  An attached plant stays ignored: both chains step with the model.
 * TOLG_E_ARG: the conditions of tolg_policy_rollout_estimated; exactly one NULL bound; a report on a family that is not
 * attached, as tolg_policy_rollout_margins has it.  A refused call changes nothing. */
int tolg_policy_covariance_estimated(tolg_handle_t h, int32_t B, const double* d_Sigma0, const double* d_W, int32_t mask,
                                     const double* d_V, double* d_Sigma, double* d_P_post, double* d_L, double* d_var_x,
                                     double* d_var_est, double* d_var_u, double* d_pos_cov, void* stream);
int tolg_policy_rollout_estimated(tolg_handle_t h, int32_t B, int32_t S, int32_t mask, const double* d_L, const double* d_dx0,
                                  const double* d_w, const double* d_n, double* d_J, int32_t* d_status, double* d_xs_q,
                                  double* d_xs_xi, double* d_us, double* d_est_q, double* d_est_xi, void* stream);
int tolg_policy_rollout_estimated_limited(tolg_handle_t h, int32_t B, int32_t S, int32_t mask, const double* d_L,
                                          const double* d_dx0, const double* d_w, const double* d_n, const double* d_u_lb,
                                          const double* d_u_ub, double* d_J, int32_t* d_status, double* d_xs_q, double* d_xs_xi,
                                          double* d_us, double* d_est_q, double* d_est_xi, int32_t* d_n_sat, double* d_u_excess,
                                          double* d_clear, int32_t* d_clear_knot, double* d_pose_margin, int32_t* d_pose_knot,
                                          int32_t* d_viol_pos, int32_t* d_viol_pose, void* stream);

/* Output feedback inside the receding-horizon loop: the filter of the two calls above, one knot at a time, with its (x^, P)
 * carried by the caller from step to step.  A step of the loop is: measure at the world knot, solve from the posterior
 * estimate, advance.  Both calls are O(B).  The conventions are those above: error coordinates, twist order [omega, v], right
 * perturbation, the 12-bit mask, d_V [B][12] read on measured coordinates only, the SO3-family rule with zeros in the
 * embedding's unused coordinates.  The actuator model (the actuated forms of the rollout and the advance) stays out of scope for output
 * feedback, here as above.
 *
 * tolg_mpc_measure: the filter's update at one world knot, on the caller's buffers alone.
 *   y = x (+) n
 *   r[j] = ([Log(q^^-1 q_y); xi_y - xi^])[j] for measured j, 0 otherwise
 *   for each measured j ascending: s = P[j][j] + V[j], c = P[:, j], P -= c c^T / s
 *   L[:, j] = P^+[:, j] / V[j] (measured j), 0 (unmeasured j)
 *   x^ <- x^ (+) L r, the pose re-normalised as the rollouts do
 *   in : mask, d_V above; d_x_q [B][16], d_x_xi [B][6] the true state; d_n [B][12] measurement noise or NULL (= 0)
 *   in/out: d_est_q [B][16], d_est_xi [B][6]   prior in, posterior out
 *           d_P [B][12][12]                    prior in (upper triangle read), posterior out, mirrored: equal to its
 *                                              transpose to the bit
 *   out: d_L [B][12][12], d_innov [B][12] (r), d_var_est [B][12] (diag P^+, the bits of d_P's diagonal); each may be NULL.
 * mask == 0 leaves the estimate bit for bit, gives L = 0 and r = 0, and P is its mirrored upper triangle.  A trajectory's bits
 * depend on neither B nor its neighbours.  The call needs no held policy and touches none; it does not read the workspace and
 * is legal during a solve in flight.
 * TOLG_E_ARG: B outside 1..max_batch; a bad mask (above); a NULL d_V with mask != 0; a NULL state, estimate or d_P.  A refused
 * call changes nothing.
 *
 * tolg_mpc_advance_estimated: tolg_mpc_advance_limited for a loop whose solve began from the posterior estimate, so that x*_0 of
 * the held policy IS that estimate: a solve keeps x*_0 = x0 to the bit in both modes (single and multiple shooting), whether
 * it converged or stopped at max_iter.  (In the workspace's own representation: the pose is held as a unit quaternion, and a
 * [16] matrix that passes through it comes back equal to rounding, not to the bit -- xs_q[0] of tolg_solve_end is the round
 * trip of d_x0_q, the same bits for every solve that began from it; the twist comes back to the bit.)
 *   u = clamp(u*_0), the three-way select of tolg_mpc_advance_limited; d_u_lb, d_u_ub [B][m], both or neither (no clamp)
 *   the true state, in place: x_true <- f(x_true, u) on plant row b where tolg_set_plant is attached with S = 1, else on the
 *     model; then xi_true += w[b]
 *   the estimate's prior: x_next = f(x*_0, u) on the MODEL, always, and w is not added (the filter knows the applied input and
 *     not the disturbance); xs_warm[0] = x_next; the tail xs_warm[N] and us_warm are those of tolg_mpc_advance
 *   the covariance, in place: P <- A P A^T + E W E^T, A = f_x(x*_0, u*_0) linearised by this call at the held nominal exactly
 *     as tolg_policy_covariance_estimated does, E = [0; I6]; d_W [B][6][6] or NULL (= 0); upper triangles read, the result
 *     mirrored to the bit; P = 0 with d_W NULL stays exact zeros
 *   d_J_cl[b] += l(x_true before the step, u) at knot 0 of the window, under the tracking-cost rules of tolg_mpc_advance
 *   d_n_sat as in tolg_mpc_advance_limited; 0 without a box
 *   in : d_w [B][6] or NULL; the box; d_W
 *   in/out: d_x_true_q [B][16], d_x_true_xi [B][6], d_P [B][12][12]: required
 *   out: d_x_next_q, d_x_next_xi, d_u_applied, d_J_cl, d_n_sat: each may be NULL; the three warm buffers: required.
 * Without a plant and with d_w NULL, x_next, u_applied, the warm start and n_sat are the bits of tolg_mpc_advance_limited;
 * with x_true = x*_0 to the bit, x_true and the increment of J_cl are those of its x_next and J_cl (plant and w included).  The
 * held policy is left alone: a second call with x_true and P restored gives the same bits.  A trajectory's bits depend on
 * neither B nor its neighbours.
 * TOLG_E_ARG: the conditions of tolg_mpc_advance_limited, except that both bounds may be NULL (exactly one is refused); a NULL
 * d_x_true_q, d_x_true_xi or d_P.  A refused call changes nothing.
 * Cost on an MI355X: INTEGRATION.md 3u. */
int tolg_mpc_measure(tolg_handle_t h, int32_t B, int32_t mask, const double* d_V, const double* d_x_q, const double* d_x_xi,
                     const double* d_n, double* d_est_q, double* d_est_xi, double* d_P, double* d_L, double* d_innov,
                     double* d_var_est, void* stream);
int tolg_mpc_advance_estimated(tolg_handle_t h, int32_t B, const double* d_w, const double* d_u_lb, const double* d_u_ub,
                               double* d_x_true_q, double* d_x_true_xi, double* d_P, const double* d_W, double* d_x_next_q,
                               double* d_x_next_xi, double* d_u_applied, double* d_xs_q_warm, double* d_xs_xi_warm,
                               double* d_us_warm, double* d_J_cl, int32_t* d_n_sat, void* stream);

/* Plants: per-sample dynamics parameters that step the closed loops of tolg_policy_rollout and tolg_mpc_advance in place of
 * the model's (model mismatch: a payload change, a mis-identified inertia, domain randomisation).  The planner's model stays
 * the handle's tolg_problem, and so do dt, gravity, kind, m, the input map, the cost, the reference and the weights.
 *   in : d_J [B][S][36] row-major 6x6 blkdiag(Ib, Jv), SPD, under the rule of tolg_problem.J (SO3 family: blkdiag(J_so3, I3));
 *        d_pend [B][S][2] (pend_mass, pend_length) for TOLG_DYN_PENDULUM3D, NULL for every other kind.
 *   form: TOLG_PLANT_DIAG is the caller's promise that every block is diagonal (only the diagonals are read);
 *         TOLG_PLANT_DENSE takes any blkdiag(Ib, Jv), diagonal ones included.
 * Row (b, s) derives Ibinv, Jvinv, Bt = Ibinv dt, mass = J[4][4], mass * grav and pend_k = pend_mass * pend_length / 2 as
 * tolg_create derives the model's; the diagonal form's inverses are the correctly rounded 1.0 / d, so a diagonal plant equal
 * to the model steps with the model's bits.  The rows are packed into the caller-owned d_packed (field-major over the B S
 * rows, packed_bytes >= tolg_plant_bytes(prob, B, S)), which the handle reads until the plant is detached (d_J = NULL).
 * While a plant is set:
 *   tolg_policy_rollout(B, S') steps sample (b, s) with row (b, s) when S == S', with row (b, 0) for every sample when S == 1;
 *     another S' or another B is TOLG_E_ARG.  Control law, noise and cost are unchanged: J is the tracking cost of the
 *     trajectory the plant produced;
 *   tolg_mpc_advance requires S == 1 (else TOLG_E_ARG): x_next (and xs_warm[0]) steps plant row b; the warm tail
 *     xs_warm[N] = f(x*_N, u*_{N-1}) is the model's prediction; u_applied and J_cl are unchanged.
 * Every other entry point ignores the plant (the same bits as with none).  It survives solves, tolg_set_refs and
 * tolg_set_weights; tolg_create starts without one; tolg_set_plant leaves the held policy.
 * TOLG_E_ARG: a solve in flight, B < 1 or B > max_batch, S < 1, an unknown form, a NULL or too small d_packed, a NULL d_pend
 * for the pendulum or a non-NULL one for any other kind. */
enum { TOLG_PLANT_DIAG = 0, TOLG_PLANT_DENSE = 1 };
size_t tolg_plant_bytes(const tolg_problem* prob, int32_t max_batch, int32_t S);
int tolg_set_plant(tolg_handle_t h, int32_t B, int32_t S, int32_t form, const double* d_J, const double* d_pend,
                   double* d_packed, size_t packed_bytes, void* stream);

/* Timing hook for bench.py: HIP-event time (ms) and launch count of the dominant kernel
 * (backward sweep) accumulated since the last call with reset != 0.  Synchronises the recorded
 * events only.  Timing is not free: an event pair per launch lengthens an accept-always iteration
 * (two launches) by ~11 us of 600 on an MI355X -- leave it off where the rate matters (default). */
int tolg_kernel_time(tolg_handle_t h, int32_t reset, double* ms_backward, double* ms_rollout,
                     double* ms_linearize, int64_t* launches);
void tolg_enable_timing(tolg_handle_t h, int32_t on);

const char* tolg_version(void);

/* Diagnostic (no reference counterpart): the series forms of the Lie primitives (csrc/tolg_lie.h: se3_exp_fast,
 * se3_log_fast, so3_coef_fast, ljacinv_coef_fast, so3_exp_fast) evaluated one lane per argument set, under the
 * wave-shared gates their callers build -- so that arguments on both sides of every tier / domain boundary share a
 * wavefront -- for the parity test of those forms against a long-double reference (tests/test_gpu_series.py).
 *   in : d_args [n][8] = rotation vector w (3), translation part v (3), th2 of a second (step) rotation, mode
 *        (0: every function under its own gate, 1: one gate for all, built as lin_knot builds it)
 *   out: d_out [n][24] = so3_coef_fast a b c1 c2 c3 | ljacinv_coef_fast | se3_exp_fast q(4) t(3) |
 *        se3_log_fast(se3_exp(w, v)) w(3) v(3) | so3_exp_fast(w) q(4) | so3_coef_fast(th2_step).a
 * n must be a multiple of 64. */
int tolg_selftest_series(int32_t n, const double* d_args, double* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TOLG_H */
