"""ctypes binding of include/tolg.h (the drop-in boundary).  Plain pointers and sizes only."""
import ctypes as C
import os

from ._build import lib_path

DYN_SE3, DYN_RIGIDBODY, DYN_DRONE, DYN_SO3, DYN_PENDULUM3D = 0, 1, 2, 3, 4
MODE_MS, MODE_SS = 0, 1
ST_OK, ST_MAXREG, ST_NODESCENT, ST_NONFINITE, ST_INTERNAL = 0, 1, 2, 3, 4
SCHED_AUTO, SCHED_SPLIT = 0, 1
MAX_OBSTACLES = 16  # TOLG_MAX_OBSTACLES
OBS_KEEP_OUT, OBS_KEEP_IN, OBS_HALF_SPACE, OBS_COLUMN_Z = 0, 1, 2, 3  # TOLG_OBS_*
MAX_POSE_CONSTRAINTS = 8  # TOLG_MAX_POSE_CONSTRAINTS
POSE_TILT_CONE, POSE_VIEW_CONE = 0, 1  # TOLG_POSE_*
BOX_PER_TRAJECTORY, BOX_PER_KNOT = 1, 2  # TOLG_BOX_*
PLANT_DIAG, PLANT_DENSE = 0, 1
MAX_ACT_DELAY = 4  # TOLG_MAX_ACT_DELAY
_ERR = {-1: "bad argument", -2: "workspace too small", -3: "kernel launch failed", -4: "inertia matrix singular"}


class Problem(C.Structure):
    _fields_ = [("kind", C.c_int32), ("m", C.c_int32), ("N", C.c_int32), ("reserved", C.c_int32),
                ("dt", C.c_double), ("J", C.c_double * 36), ("Q", C.c_double * 144), ("P", C.c_double * 144),
                ("R", C.c_double * 36), ("pend_mass", C.c_double), ("pend_length", C.c_double)]


class Options(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_iter", C.c_int32), ("line_search", C.c_int32),
                ("rollout_linear", C.c_int32), ("tol_grad", C.c_double), ("tol_defect", C.c_double),
                ("max_reg", C.c_double), ("schedule", C.c_int32), ("check_every", C.c_int32)]


class Actuator(C.Structure):
    """tolg_actuator: device pointers [B][m] (0: the default of the header) and the delay in knots."""
    _fields_ = [("d_lb", C.c_void_p), ("d_ub", C.c_void_p), ("d_beta", C.c_void_p), ("d_du_max", C.c_void_p),
                ("d_u_init", C.c_void_p), ("delay", C.c_int32)]


_lib = None
SYMBOLS = ["tolg_workspace_bytes", "tolg_create", "tolg_destroy", "tolg_solve_batch", "tolg_solve_begin",
           "tolg_solve_iterate", "tolg_solve_iterate_until", "tolg_solve_end", "tolg_solve_peek", "tolg_solve_active_count", "tolg_set_al", "tolg_set_al_box", "tolg_set_al_box_windows", "tolg_al_update",
           "tolg_refs_bytes", "tolg_set_refs", "tolg_weights_bytes", "tolg_set_weights",
           "tolg_pose_schedule_bytes", "tolg_set_pose_schedule", "tolg_set_pose_schedule_windows", "tolg_eval_knot", "tolg_linearize_backward",
           "tolg_rollout", "tolg_expected_change", "tolg_solve_gains", "tolg_policy_rollout",
           "tolg_solve_begin_warm", "tolg_set_ref_windows", "tolg_mpc_advance", "tolg_obstacles_bytes", "tolg_set_al_obstacles", "tolg_obstacles_moving_bytes", "tolg_set_al_obstacles_moving",
           "tolg_al_update_state", "tolg_al_mpc_step", "tolg_set_al_obstacle_windows", "tolg_set_al_obstacle_kinds", "tolg_pose_constraints_bytes", "tolg_set_al_pose_constraints",
           "tolg_set_al_pose_constraint_windows", "tolg_al_mpc_step_pose", "tolg_plant_bytes", "tolg_set_plant", "tolg_policy_covariance", "tolg_policy_value", "tolg_policy_covariance_estimated", "tolg_policy_rollout_estimated", "tolg_policy_rollout_limited", "tolg_mpc_advance_limited",
           "tolg_policy_rollout_margins", "tolg_policy_rollout_estimated_limited", "tolg_policy_rollout_actuated",
           "tolg_mpc_advance_actuated", "tolg_mpc_measure", "tolg_mpc_advance_estimated", "tolg_kernel_time", "tolg_enable_timing", "tolg_version", "tolg_selftest_series"]


def load():
    """Load libtolg_hip.so or raise: the product has no CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    so = lib_path()
    if not os.path.exists(so):
        raise RuntimeError(
            "HIP extension %s is missing. Build it with "
            "trajectory_optimization_matrix_lie_groups_amd.build_extension() (needs hipcc); "
            "there is no CPU fallback." % so)
    lib = C.CDLL(so)
    vp, dp, ip = C.c_void_p, C.c_void_p, C.c_void_p
    lib.tolg_workspace_bytes.restype = C.c_size_t
    lib.tolg_workspace_bytes.argtypes = [C.POINTER(Problem), C.c_int32]
    lib.tolg_create.restype = C.c_int
    lib.tolg_create.argtypes = [C.POINTER(Problem), dp, dp, C.c_int32, vp, C.c_size_t, vp, C.POINTER(vp)]
    lib.tolg_destroy.restype = None
    lib.tolg_destroy.argtypes = [vp]
    lib.tolg_solve_batch.restype = C.c_int
    lib.tolg_solve_batch.argtypes = [vp, C.POINTER(Options), C.c_int32] + [dp] * 11 + [ip] * 3 + [vp]
    lib.tolg_solve_begin.restype = C.c_int
    lib.tolg_solve_begin.argtypes = [vp, C.POINTER(Options), C.c_int32] + [dp] * 8 + [vp]
    lib.tolg_solve_iterate.restype = C.c_int
    lib.tolg_solve_iterate.argtypes = [vp, C.c_int32, vp]
    lib.tolg_solve_iterate_until.restype = C.c_int
    lib.tolg_solve_iterate_until.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), vp]
    lib.tolg_solve_end.restype = C.c_int
    lib.tolg_solve_end.argtypes = [vp, dp, dp, dp, ip, ip, ip, vp]
    lib.tolg_solve_peek.restype = C.c_int
    lib.tolg_solve_peek.argtypes = [vp, dp, dp, dp, ip, ip, ip, vp]
    lib.tolg_solve_active_count.restype = C.c_int
    lib.tolg_solve_active_count.argtypes = [vp, ip, vp]
    lib.tolg_set_al.restype = C.c_int
    lib.tolg_set_al.argtypes = [vp, dp, dp, dp, dp]
    lib.tolg_set_al_box.restype = C.c_int
    lib.tolg_set_al_box.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp]
    lib.tolg_set_al_box_windows.restype = C.c_int
    lib.tolg_set_al_box_windows.argtypes = [vp, C.c_int32, dp, dp, C.c_int32, ip, C.c_int32, dp, dp, dp, dp, vp]
    lib.tolg_refs_bytes.restype = C.c_size_t
    lib.tolg_refs_bytes.argtypes = [C.POINTER(Problem), C.c_int32]
    lib.tolg_set_refs.restype = C.c_int
    lib.tolg_set_refs.argtypes = [vp, C.c_int32, dp, dp, vp, C.c_size_t, vp]
    lib.tolg_weights_bytes.restype = C.c_size_t
    lib.tolg_weights_bytes.argtypes = [C.POINTER(Problem), C.c_int32]
    lib.tolg_set_weights.restype = C.c_int
    lib.tolg_set_weights.argtypes = [vp, C.c_int32, dp, dp, dp, vp, C.c_size_t, vp]
    lib.tolg_pose_schedule_bytes.restype = C.c_size_t
    lib.tolg_pose_schedule_bytes.argtypes = [C.POINTER(Problem), C.c_int32]
    lib.tolg_set_pose_schedule.restype = C.c_int
    lib.tolg_set_pose_schedule.argtypes = [vp, C.c_int32, dp, vp, C.c_size_t, vp]
    lib.tolg_set_pose_schedule_windows.restype = C.c_int
    lib.tolg_set_pose_schedule_windows.argtypes = [vp, C.c_int32, dp, C.c_int32, ip, C.c_int32, vp, C.c_size_t, vp]
    lib.tolg_al_update.restype = C.c_int
    lib.tolg_al_update.argtypes = [vp, C.c_int32, dp, dp, dp, dp, dp, dp, C.c_double, C.c_double, C.c_double, dp, ip, vp]
    lib.tolg_eval_knot.restype = C.c_int
    lib.tolg_eval_knot.argtypes = [vp, C.c_int32, C.c_int32] + [dp] * 13 + [vp]
    lib.tolg_linearize_backward.restype = C.c_int
    lib.tolg_linearize_backward.argtypes = [vp, C.c_int32, C.c_double, C.c_int32] + [dp] * 13 + [vp]
    lib.tolg_rollout.restype = C.c_int
    lib.tolg_rollout.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, dp, dp, dp, vp]
    lib.tolg_expected_change.restype = C.c_int
    lib.tolg_expected_change.argtypes = [vp, C.c_int32, C.c_int32, dp, ip, vp]
    lib.tolg_solve_gains.restype = C.c_int
    lib.tolg_solve_gains.argtypes = [vp, C.c_int32, dp, dp, vp]
    lib.tolg_policy_rollout.restype = C.c_int
    lib.tolg_policy_rollout.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, ip, dp, dp, dp, vp]
    lib.tolg_solve_begin_warm.restype = C.c_int
    lib.tolg_solve_begin_warm.argtypes = [vp, C.POINTER(Options), C.c_int32] + [dp] * 10 + [vp]
    lib.tolg_set_ref_windows.restype = C.c_int
    lib.tolg_set_ref_windows.argtypes = [vp, C.c_int32, dp, dp, C.c_int32, ip, C.c_int32, vp, C.c_size_t, vp]
    lib.tolg_mpc_advance.restype = C.c_int
    lib.tolg_mpc_advance.argtypes = [vp, C.c_int32] + [dp] * 8 + [vp]
    lib.tolg_obstacles_bytes.restype = C.c_size_t
    lib.tolg_obstacles_bytes.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32]
    lib.tolg_set_al_obstacles.restype = C.c_int
    lib.tolg_set_al_obstacles.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, vp, C.c_size_t, vp]
    lib.tolg_obstacles_moving_bytes.restype = C.c_size_t
    lib.tolg_obstacles_moving_bytes.argtypes = lib.tolg_obstacles_bytes.argtypes
    lib.tolg_set_al_obstacles_moving.restype = C.c_int
    lib.tolg_set_al_obstacles_moving.argtypes = lib.tolg_set_al_obstacles.argtypes
    lib.tolg_al_update_state.restype = C.c_int
    lib.tolg_al_update_state.argtypes = [vp, C.c_int32, dp, dp, dp, C.c_double, C.c_double, C.c_double, dp, ip, vp]
    lib.tolg_al_mpc_step.restype = C.c_int
    lib.tolg_al_mpc_step.argtypes = [vp, C.c_int32, dp, dp, dp, C.c_double, C.c_double, C.c_double, dp, C.c_int32, vp]
    lib.tolg_al_mpc_step_pose.restype = C.c_int
    lib.tolg_al_mpc_step_pose.argtypes = lib.tolg_al_mpc_step.argtypes
    lib.tolg_set_al_obstacle_windows.restype = C.c_int
    lib.tolg_set_al_obstacle_windows.argtypes = [vp, C.c_int32, C.c_int32, dp, C.c_int32, ip, C.c_int32, dp, dp, vp, C.c_size_t, vp]
    lib.tolg_set_al_obstacle_kinds.restype = C.c_int
    lib.tolg_set_al_obstacle_kinds.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), vp]
    lib.tolg_pose_constraints_bytes.restype = C.c_size_t
    lib.tolg_pose_constraints_bytes.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32, C.c_int32]
    lib.tolg_set_al_pose_constraints.restype = C.c_int
    lib.tolg_set_al_pose_constraints.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), dp, C.c_int32, dp, dp, vp, C.c_size_t, vp]
    lib.tolg_set_al_pose_constraint_windows.restype = C.c_int
    lib.tolg_set_al_pose_constraint_windows.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), dp, C.c_int32, ip, C.c_int32, dp, dp,
                                                        vp, C.c_size_t, vp]
    lib.tolg_plant_bytes.restype = C.c_size_t
    lib.tolg_plant_bytes.argtypes = [C.POINTER(Problem), C.c_int32, C.c_int32]
    lib.tolg_set_plant.restype = C.c_int
    lib.tolg_set_plant.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, dp, dp, C.c_size_t, vp]
    lib.tolg_policy_covariance.restype = C.c_int
    lib.tolg_policy_covariance.argtypes = [vp, C.c_int32, dp, dp, dp, dp, dp, dp, vp]
    lib.tolg_policy_value.restype = C.c_int
    lib.tolg_policy_value.argtypes = [vp, C.c_int32, dp, dp, dp, dp, dp, dp, dp, vp]
    lib.tolg_policy_covariance_estimated.restype = C.c_int
    lib.tolg_policy_covariance_estimated.argtypes = [vp, C.c_int32, dp, dp, C.c_int32] + [dp] * 8 + [vp]
    lib.tolg_policy_rollout_estimated.restype = C.c_int
    lib.tolg_policy_rollout_estimated.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, ip, dp, dp, dp, dp, dp, vp]
    lib.tolg_policy_rollout_limited.restype = C.c_int
    lib.tolg_policy_rollout_limited.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, ip, dp, dp, dp, ip, dp, dp, ip, vp]
    lib.tolg_policy_rollout_margins.restype = C.c_int
    lib.tolg_policy_rollout_margins.argtypes = lib.tolg_policy_rollout_limited.argtypes[:-1] + [dp, ip, ip, ip, vp]
    lib.tolg_policy_rollout_estimated_limited.restype = C.c_int
    lib.tolg_policy_rollout_estimated_limited.argtypes = (lib.tolg_policy_rollout_estimated.argtypes[:8] + [dp, dp]
                                                          + lib.tolg_policy_rollout_estimated.argtypes[8:-1]
                                                          + [ip, dp, dp, ip, dp, ip, ip, ip, vp])
    lib.tolg_mpc_advance_limited.restype = C.c_int
    lib.tolg_mpc_advance_limited.argtypes = [vp, C.c_int32] + [dp] * 10 + [ip, vp]
    lib.tolg_policy_rollout_actuated.restype = C.c_int
    lib.tolg_policy_rollout_actuated.argtypes = ([vp, C.c_int32, C.c_int32, dp, dp, C.POINTER(Actuator)]
                                                 + lib.tolg_policy_rollout_margins.argtypes[7:-1] + [dp, ip, dp, vp])
    lib.tolg_mpc_advance_actuated.restype = C.c_int
    lib.tolg_mpc_advance_actuated.argtypes = [vp, C.c_int32, dp, C.POINTER(Actuator)] + [dp] * 8 + [ip, ip, vp]
    lib.tolg_mpc_measure.restype = C.c_int
    lib.tolg_mpc_measure.argtypes = [vp, C.c_int32, C.c_int32] + [dp] * 10 + [vp]
    lib.tolg_mpc_advance_estimated.restype = C.c_int
    lib.tolg_mpc_advance_estimated.argtypes = [vp, C.c_int32] + [dp] * 14 + [ip, vp]
    lib.tolg_kernel_time.restype = C.c_int
    lib.tolg_kernel_time.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.tolg_enable_timing.restype = None
    lib.tolg_enable_timing.argtypes = [vp, C.c_int32]
    lib.tolg_version.restype = C.c_char_p
    lib.tolg_version.argtypes = []
    lib.tolg_selftest_series.restype = C.c_int
    lib.tolg_selftest_series.argtypes = [C.c_int32, dp, dp, vp]
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s (rc=%d)" % (what, _ERR.get(rc, "unknown"), rc))
