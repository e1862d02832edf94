"""ctypes binding of libgmr_amd.so (the C ABI in include/gmr_amd.h).

Fails loudly: if the shared library is missing or does not export the expected ABI,
importing anything that needs it raises -- there is no Python/CPU fallback path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .build import LIB_PATH as _DEFAULT_LIB_PATH

LIB_PATH = os.environ.get("GMR_AMD_LIB") or _DEFAULT_LIB_PATH  # override only for A/B diagnostics of variant builds

ABI_VERSION = 5
GMR_DTYPE_F32, GMR_DTYPE_F64 = 0, 1

WORK_ITEM_DTYPE = np.dtype(
    [("frame_begin", "<i8"), ("n_burn", "<i4"), ("n_out", "<i4"), ("init_row", "<i4"), ("final_row", "<i4"),
     ("burn_row", "<i4"), ("check_stride", "<i4"), ("height_scale", "<f8")], align=True
)
assert WORK_ITEM_DTYPE.itemsize == 40
INIT_QPOS0, INIT_ROOT_TARGET = -1, -2

EXPORTS = ["gmr_abi_version", "gmr_model_create", "gmr_model_destroy", "gmr_last_error", "gmr_model_info_get",
           "gmr_ik_solve", "gmr_fk", "gmr_fk_shape", "gmr_dof_to_rot", "gmr_rot_to_dof", "gmr_local_rot_to_global", "gmr_fk_min_height", "gmr_bvh_fk", "gmr_bvh_parse_header", "gmr_bvh_parse_motion", "gmr_evaluate", "gmr_smplx_keypoints", "gmr_smplx_keypoints_cols", "gmr_smplx_keypoints_in", "gmr_smplx_body", "gmr_bvh_fk_rows", "gmr_bvh_parse_motion_device",
           "gmr_session_create", "gmr_session_destroy", "gmr_session_reset", "gmr_session_step", "gmr_session_state", "gmr_session_set_persistent", "gmr_ik_plan_order", "gmr_ik_solve_ordered",
           "gmr_group_create", "gmr_group_destroy", "gmr_group_size", "gmr_group_model", "gmr_group_last_error", "gmr_group_ik_solve",
           "gmr_group_plan_order", "gmr_group_ik_solve_ordered", "gmr_motion_epilogue", "gmr_group_motion_epilogue",
           "gmr_clip_report", "gmr_group_clip_report", "gmr_motion_track", "gmr_group_motion_track",
           "gmr_model_set_step_cap", "gmr_model_get_step_cap", "gmr_motion_sample", "gmr_lowpass_coefficients",
           "gmr_ik_balance_plan", "gmr_ik_sliced_timeouts", "gmr_motion_contacts", "gmr_motion_footlock", "gmr_motion_dynamics",
           "gmr_motion_self_collision", "gmr_motion_mirror", "gmr_motion_compose", "gmr_motion_transitions",
           "gmr_motion_retime_plan", "gmr_motion_retime_apply", "gmr_motion_retime_plan_torque",
           "gmr_motion_self_collision_repair"]


class IKParams(C.Structure):
    """``gmr_ik_params`` (include/gmr_blob.h); defaults = the reference's constants."""

    _fields_ = [
        ("damping", C.c_double), ("tol", C.c_double), ("limit_gain", C.c_double), ("lm_damping", C.c_double),
        ("max_iter", C.c_int32), ("offset_to_ground", C.c_int32), ("check_tol", C.c_double),
    ]

    def __init__(self, damping=0.5, tol=1e-3, limit_gain=0.95, lm_damping=1.0, max_iter=10, offset_to_ground=0, check_tol=1e-7):
        super().__init__(float(damping), float(tol), float(limit_gain), float(lm_damping), int(max_iter), int(offset_to_ground),
                         float(check_tol))


class ModelInfo(C.Structure):
    _fields_ = [
        ("nbody", C.c_int32), ("nq", C.c_int32), ("nv", C.c_int32), ("nslot", C.c_int32), ("ntask", C.c_int32 * 2),
        ("n_active_dof", C.c_int32), ("nv_padded", C.c_int32), ("lds_bytes", C.c_int32), ("device", C.c_int32),
        ("reserved", C.c_int32 * 6),
    ]


class GroupInput(C.Structure):
    """``gmr_group_input`` (include/gmr_amd.h): one member's arguments of a group launch."""

    _fields_ = [
        ("human_pos", C.c_void_p), ("human_quat", C.c_void_p), ("in_dtype", C.c_int32), ("n_cols", C.c_int32),
        ("slot_col", C.c_void_p), ("n_frames", C.c_int64), ("items", C.c_void_p), ("n_items", C.c_int32), ("reserved", C.c_int32),
        ("qpos_init", C.c_void_p), ("qpos_final", C.c_void_p), ("qpos_out", C.c_void_p), ("iters_out", C.c_void_p), ("frames_done", C.c_void_p),
    ]


MOTION_HEIGHT_ADJUST, MOTION_ROOT_ORIGIN = 1, 2


class MotionInput(C.Structure):
    """``gmr_motion_input`` (include/gmr_amd.h): one model's arguments of the dataset epilogue."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("n_seq", C.c_int32), ("flags", C.c_int32),
        ("ground_offset", C.c_double), ("root_pos_out", C.c_void_p), ("root_rot_out", C.c_void_p), ("dof_pos_out", C.c_void_p),
        ("local_body_pos_out", C.c_void_p), ("min_z_out", C.c_void_p),
    ]


TRACK_OUTPUTS = ("root_pos", "root_rot", "joint_pos", "root_lin_vel", "root_ang_vel", "joint_vel",
                 "body_pos_w", "body_quat_w", "body_lin_vel_w", "body_ang_vel_w")  # gmr_track_input's output pointers, in order


class TrackInput(C.Structure):
    """``gmr_track_input`` (include/gmr_amd.h): one model's arguments of the tracking export."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("out_offsets", C.c_void_p), ("ratio", C.c_void_p),
        ("fps_out", C.c_double), ("n_seq", C.c_int32), ("lowpass_hz", C.c_float),
    ] + [(k + "_out", C.c_void_p) for k in TRACK_OUTPUTS]


class SampleInput(C.Structure):
    """``gmr_sample_input`` (include/gmr_amd.h): the arguments of one motion-library query call."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("fps", C.c_void_p),
        ("n_seq", C.c_int32), ("k_per_id", C.c_int32), ("ids", C.c_void_p), ("times", C.c_void_p),
        ("time_dtype", C.c_int32), ("out_dtype", C.c_int32), ("n_queries", C.c_int64),
        ("body_ids", C.c_void_p), ("n_sel", C.c_int32), ("reserved", C.c_int32),
    ] + [(k + "_out", C.c_void_p) for k in TRACK_OUTPUTS]


CONTACT_GROUND_FIXED, CONTACT_GROUND_CLIP_MIN = 0, 1   # GMR_CONTACT_GROUND_* (include/gmr_amd.h)
CONTACT_MAX_BODIES = 64
CONTACT_OUTPUTS = ("contact", "frames", "touchdowns", "slide_sum", "slide_step_max", "depth_max", "airborne_frames", "base")  # gmr_contact_input's output pointers, in order


class ContactInput(C.Structure):
    """``gmr_contact_input`` (include/gmr_amd.h): the whole call of the contact labels, its stream included."""

    _fields_ = [
        ("body_pos_w", C.c_void_p), ("body_lin_vel_w", C.c_void_p), ("n_rows", C.c_int64), ("out_offsets", C.c_void_p),
        ("body_ids", C.c_void_p), ("height_offset", C.c_void_p), ("n_seq", C.c_int32), ("n_contact", C.c_int32),
        ("ground_mode", C.c_int32), ("reserved", C.c_int32), ("ground_z", C.c_double),
        ("height_on", C.c_double), ("height_off", C.c_double), ("speed_on", C.c_double), ("speed_off", C.c_double),
        ("stream", C.c_void_p),
    ] + [(k + "_out", C.c_void_p) for k in CONTACT_OUTPUTS]


FOOTLOCK_MAX_BODIES, FOOTLOCK_MAX_ITERATIONS = 8, 32   # contact columns and iterations of one gmr_motion_footlock call
FOOTLOCK_OUTPUTS = ("qpos", "pos", "shift", "runs", "locked_frames", "shift_max", "residual_max", "limit_frames")  # gmr_footlock_input's output pointers, in order


class FootlockInput(C.Structure):
    """``gmr_footlock_input`` (include/gmr_amd.h): the whole call of the foot locking, its stream included.  ``body_ids`` is a
    HOST array."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("contact", C.c_void_p), ("body_ids", C.c_void_p),
        ("n_seq", C.c_int32), ("n_contact", C.c_int32), ("blend_frames", C.c_int32), ("min_run", C.c_int32),
        ("iterations", C.c_int32), ("reserved", C.c_int32), ("damping", C.c_double), ("step_cap", C.c_double),
        ("stream", C.c_void_p),
    ] + [(k + "_out", C.c_void_p) for k in FOOTLOCK_OUTPUTS]


DYNAMICS_FRAME_OUTPUTS = ("tau", "root_wrench", "com", "zmp", "qvel", "qacc")   # gmr_dynamics_input's output pointers, in order:
DYNAMICS_STATS = ("tau_abs_max", "tau_rms", "tau_ratio_max", "frames_over_limit", "frames_any_over_limit", "fz_ratio_max", "fz_ratio_min",
                  "unloaded_frames", "nonfinite_frames")                         # per frame, then per clip
DYNAMICS_OUTPUTS = DYNAMICS_FRAME_OUTPUTS + DYNAMICS_STATS
DYNAMICS_TABLE = ("body_parent", "body_mass", "body_com", "body_inertia", "armature", "torque_limit")  # the inertial table's arrays


class DynamicsInput(C.Structure):
    """``gmr_dynamics_input`` (include/gmr_amd.h): the whole call of the inverse dynamics, its stream included."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("qvel", C.c_void_p), ("qacc", C.c_void_p),
        ("n_seq", C.c_int32), ("nbody", C.c_int32), ("fps", C.c_double),
        ("gravity_x", C.c_double), ("gravity_y", C.c_double), ("gravity_z", C.c_double), ("ground_z", C.c_double), ("fz_min", C.c_double),
    ] + [(k, C.c_void_p) for k in DYNAMICS_TABLE] + [("stream", C.c_void_p)] + [(k + "_out", C.c_void_p) for k in DYNAMICS_OUTPUTS]


SELF_COLLISION_FRAME_OUTPUTS = ("clearance", "pair", "hits")   # gmr_self_collision_input's output pointers, in order: per frame,
SELF_COLLISION_STATS = ("clearance_min", "worst_frame", "worst_pair", "colliding_frames", "longest_run", "hits_sum",
                        "nonfinite_frames")                     # then per clip
SELF_COLLISION_OUTPUTS = SELF_COLLISION_FRAME_OUTPUTS + SELF_COLLISION_STATS
SELF_COLLISION_TABLE = ("cap_body", "cap_p0", "cap_p1", "cap_radius", "pairs")   # the proxy tables' arrays
SELF_COLLISION_MAX_CAPS, SELF_COLLISION_MAX_PAIRS = 256, 32768


class SelfCollisionInput(C.Structure):
    """``gmr_self_collision_input`` (include/gmr_amd.h): the whole call of the self-collision report, its stream included."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("n_seq", C.c_int32), ("n_caps", C.c_int32),
        ("n_pairs", C.c_int32), ("reserved", C.c_int32),
    ] + [(k, C.c_void_p) for k in SELF_COLLISION_TABLE] + [("margin", C.c_double), ("stream", C.c_void_p)] \
      + [(k + "_out", C.c_void_p) for k in SELF_COLLISION_OUTPUTS]


SELF_COLLISION_REPAIR_FRAME_OUTPUTS = ("qpos", "clearance_before", "clearance_after", "move")   # gmr_self_collision_repair_input's
SELF_COLLISION_REPAIR_STATS = ("repaired_frames", "unresolved_frames", "move_max", "clearance_min_after",
                               "nonfinite_frames")              # output pointers, in order: per frame, then per clip
SELF_COLLISION_REPAIR_OUTPUTS = SELF_COLLISION_REPAIR_FRAME_OUTPUTS + SELF_COLLISION_REPAIR_STATS
SELF_COLLISION_REPAIR_MAX_ITERATIONS = 32


class SelfCollisionRepairInput(C.Structure):
    """``gmr_self_collision_repair_input`` (include/gmr_amd.h): the whole call of the self-collision repair, its stream included."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("n_seq", C.c_int32), ("n_caps", C.c_int32),
        ("n_pairs", C.c_int32), ("iterations", C.c_int32),
    ] + [(k, C.c_void_p) for k in SELF_COLLISION_TABLE] \
      + [("margin", C.c_double), ("damping", C.c_double), ("step_cap", C.c_double), ("resolve_tol", C.c_double),
         ("hinge_mask", C.c_uint64), ("stream", C.c_void_p)] + [(k + "_out", C.c_void_p) for k in SELF_COLLISION_REPAIR_OUTPUTS]


MIRROR_WORLD, MIRROR_CLIP_START = 0, 1    # GMR_MIRROR_WORLD, GMR_MIRROR_CLIP_START
MIRROR_MODES = {"world": MIRROR_WORLD, "start": MIRROR_CLIP_START}
MIRROR_MAX_NQ = 64


class MirrorInput(C.Structure):
    """``gmr_mirror_input`` (include/gmr_amd.h): the whole call of the mirror augmentation, its stream included."""

    _fields_ = [("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("n_seq", C.c_int32), ("mode", C.c_int32),
                ("col_src", C.c_void_p), ("col_sign", C.c_void_p), ("stream", C.c_void_p), ("qpos_out", C.c_void_p), ("reserved", C.c_int64)]


COMPOSE_MAX_NQ = 64


class ComposeInput(C.Structure):
    """``gmr_compose_input`` (include/gmr_amd.h): the whole call of the clip composition, its stream included."""

    _fields_ = [("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seg_src", C.c_void_p), ("seg_len", C.c_void_p), ("seg_blend", C.c_void_p),
                ("seg_out", C.c_void_p), ("clip_segs", C.c_void_p), ("n_seg", C.c_int32), ("n_out", C.c_int32), ("n_out_frames", C.c_int64),
                ("stream", C.c_void_p), ("qpos_out", C.c_void_p), ("seg_transform", C.c_void_p), ("reserved", C.c_int64)]


TRANSITIONS_MAX_BODIES, TRANSITIONS_MAX_WINDOW, TRANSITIONS_MOMENTS = 64, 32, 6
TRANSITIONS_OUTPUTS = ("points", "moments", "best_cost", "best_frame", "cost_out")   # gmr_transitions_input's output pointers, in order


class TransitionsInput(C.Structure):
    """``gmr_transitions_input`` (include/gmr_amd.h): the whole call of the transition search, its stream included."""

    _fields_ = [("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("n_seq", C.c_int32), ("n_bodies", C.c_int32),
                ("body_ids", C.c_void_p), ("weights", C.c_void_p), ("window", C.c_int32), ("src_stride", C.c_int32),
                ("min_gap", C.c_int32), ("n_src_clips", C.c_int32), ("n_dst_clips", C.c_int32), ("reserved", C.c_int32),
                ("src_clips", C.c_void_p), ("src_offsets", C.c_void_p), ("dst_clips", C.c_void_p), ("dst_offsets", C.c_void_p),
                ("n_sources", C.c_int64), ("n_targets", C.c_int64), ("stream", C.c_void_p)] + [(k, C.c_void_p) for k in TRANSITIONS_OUTPUTS]


RETIME_MAX_NQ, RETIME_MAX_WINDOW, RETIME_MAX_STRETCH, RETIME_Q = 64, 32, 64.0, 1024   # kRetime* (gmr_amd/csrc/retime_kernel.hip.h)
RETIME_PLAN_OUTPUTS = ("need", "ticks", "cum", "out_len", "clip_stats", "need_max")    # gmr_retime_plan_input's output pointers, in order
RETIME_STATS = ("stretched_intervals", "capped_intervals", "nonfinite_intervals", "total_ticks")   # the columns of clip_stats


class RetimePlanInput(C.Structure):
    """``gmr_retime_plan_input`` (include/gmr_amd.h): the whole call of the retiming plan, its stream included."""

    _fields_ = [("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("n_seq", C.c_int32), ("window", C.c_int32),
                ("fps", C.c_double), ("vmax", C.c_void_p), ("max_stretch", C.c_double), ("stream", C.c_void_p)] \
        + [(k, C.c_void_p) for k in RETIME_PLAN_OUTPUTS] + [("reserved", C.c_int64)]


class RetimeApplyInput(C.Structure):
    """``gmr_retime_apply_input`` (include/gmr_amd.h): the whole call of the resampling along a retiming plan, its stream included."""

    _fields_ = [("qpos", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p), ("ticks", C.c_void_p), ("cum", C.c_void_p),
                ("out_offsets", C.c_void_p), ("n_seq", C.c_int32), ("interp", C.c_int32), ("n_out_frames", C.c_int64),
                ("stream", C.c_void_p), ("qpos_out", C.c_void_p), ("src_time", C.c_void_p)]


RETIME_INTERP = {"linear": 0, "cubic": 1}   # GMR_RETIME_INTERP_* (include/gmr_amd.h)
RETIME_TORQUE_OUTPUTS = RETIME_PLAN_OUTPUTS + ("static_over",)   # gmr_retime_torque_input's output pointers, in order


class RetimeTorqueInput(C.Structure):
    """``gmr_retime_torque_input`` (include/gmr_amd.h): the whole call of the retiming plan from joint torques, its stream included."""

    _fields_ = [("tau", C.c_void_p), ("tau_static", C.c_void_p), ("n_frames", C.c_int64), ("seq_offsets", C.c_void_p),
                ("n_seq", C.c_int32), ("window", C.c_int32), ("torque_limit", C.c_void_p), ("limit_scale", C.c_double),
                ("max_stretch", C.c_double), ("need_floor", C.c_void_p), ("align_end", C.c_int32), ("reserved", C.c_int32),
                ("stream", C.c_void_p)] + [(k, C.c_void_p) for k in RETIME_TORQUE_OUTPUTS]


CLIP_REPORT_SEGMENT = 32        # GMR_CLIP_REPORT_SEGMENT (include/gmr_amd.h)
CLIP_REPORT_LIMIT_EPS = 1e-3    # GMR_CLIP_REPORT_LIMIT_EPS


class ClipReportInput(C.Structure):
    """``gmr_clip_report_input`` (include/gmr_amd.h): one model's arguments of the clip report."""

    _fields_ = [
        ("qpos", C.c_void_p), ("n_frames", C.c_int64), ("human_pos", C.c_void_p), ("human_quat", C.c_void_p),
        ("in_dtype", C.c_int32), ("n_cols", C.c_int32), ("slot_col", C.c_void_p), ("seq_offsets", C.c_void_p),
        ("n_seq", C.c_int32), ("reserved", C.c_int32), ("height_scale", C.c_void_p), ("iters", C.c_void_p),
        ("err_max_out", C.c_void_p), ("err_sum_out", C.c_void_p),
        ("task_pos_max_out", C.c_void_p), ("task_pos_sum_out", C.c_void_p), ("task_rot_max_out", C.c_void_p), ("task_rot_sum_out", C.c_void_p),
        ("near_lo_out", C.c_void_p), ("near_hi_out", C.c_void_p),
        ("dof_step_max_out", C.c_void_p), ("root_step_max_out", C.c_void_p), ("root_turn_max_out", C.c_void_p),
        ("solves_max_out", C.c_void_p), ("solves_sum_out", C.c_void_p), ("nonfinite_frames_out", C.c_void_p),
    ]


class ClipReportParams(C.Structure):
    """``gmr_clip_report_params`` (include/gmr_amd.h)."""

    _fields_ = [("limit_eps", C.c_double), ("segment_frames", C.c_int32), ("offset_to_ground", C.c_int32)]

    def __init__(self, limit_eps=CLIP_REPORT_LIMIT_EPS, segment_frames=0, offset_to_ground=0):
        super().__init__(float(limit_eps), int(segment_frames), int(offset_to_ground))


class SmplxBodyClip(C.Structure):
    """``gmr_smplx_body_clip`` (include/gmr_amd.h): one clip's arguments of the body-model launch."""

    _fields_ = [
        ("root_orient", C.c_void_p), ("pose_body", C.c_void_p), ("trans", C.c_void_p), ("j_template", C.c_void_p), ("j_dirs", C.c_void_p),
        ("hand_mean", C.c_void_p), ("betas", C.c_void_p), ("n_frames", C.c_int64), ("in_dtype", C.c_int32 * 3), ("n_betas", C.c_int32),
        ("dirs_stride", C.c_int32), ("reserved", C.c_int32),
    ]


class IKStats(C.Structure):
    _fields_ = [("n_items", C.c_int64), ("n_frames_total", C.c_int64), ("n_frames_out", C.c_int64), ("reserved", C.c_int32 * 4)]


class NativeLibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Return the loaded library, raising ``NativeLibraryError`` if it is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m gmr_amd.build` (hipcc, gfx950). "
            "gmr_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS if not hasattr(L, s)]
    if missing:
        raise NativeLibraryError(f"{LIB_PATH} does not export {missing}")
    vp = C.c_void_p
    L.gmr_abi_version.restype = C.c_int
    if L.gmr_abi_version() != ABI_VERSION:
        raise NativeLibraryError(f"ABI version mismatch: library {L.gmr_abi_version()}, binding {ABI_VERSION}")
    L.gmr_model_create.restype = vp
    L.gmr_model_create.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, C.c_size_t]
    L.gmr_model_destroy.argtypes = [vp]
    L.gmr_last_error.restype = C.c_char_p
    L.gmr_last_error.argtypes = [vp]
    L.gmr_model_info_get.argtypes = [vp, C.POINTER(ModelInfo)]
    L.gmr_model_set_step_cap.restype = C.c_int
    L.gmr_model_set_step_cap.argtypes = [vp, vp]
    L.gmr_model_get_step_cap.restype = C.c_int
    L.gmr_model_get_step_cap.argtypes = [vp, vp]
    batch = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int, C.POINTER(IKParams), vp]  # model .. qpos_init of the three IK calls
    solve = batch + [vp, vp, vp, vp, C.POINTER(IKStats)]                                          # qpos_final .. stats
    L.gmr_ik_solve.argtypes = solve + [vp]
    L.gmr_ik_balance_plan.restype = C.c_int
    L.gmr_ik_balance_plan.argtypes = [vp, C.c_int, C.c_int]
    L.gmr_ik_sliced_timeouts.restype = C.c_int
    L.gmr_ik_sliced_timeouts.argtypes = [vp]
    L.gmr_ik_solve_ordered.argtypes = solve + [vp, vp]
    L.gmr_ik_plan_order.argtypes = batch + [C.c_int, vp, vp]
    L.gmr_group_ik_solve.argtypes = [vp, C.POINTER(GroupInput), C.POINTER(IKParams), vp]
    L.gmr_group_ik_solve_ordered.argtypes = [vp, C.POINTER(GroupInput), C.POINTER(IKParams), vp, vp]
    L.gmr_group_plan_order.argtypes = [vp, C.POINTER(GroupInput), C.POINTER(IKParams), C.c_int, vp, vp]
    for f in ("gmr_ik_solve", "gmr_ik_solve_ordered", "gmr_ik_plan_order", "gmr_group_ik_solve", "gmr_group_ik_solve_ordered", "gmr_group_plan_order"):
        getattr(L, f).restype = C.c_int
    L.gmr_fk.restype = C.c_int
    L.gmr_fk.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, vp]
    L.gmr_fk_shape.restype = C.c_int
    L.gmr_fk_shape.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int64, vp, vp, vp]
    for f in ("gmr_dof_to_rot", "gmr_rot_to_dof", "gmr_local_rot_to_global"):
        getattr(L, f).restype = C.c_int
        getattr(L, f).argtypes = [vp, vp, C.c_int64, vp, vp]
    L.gmr_fk_min_height.restype = C.c_int
    L.gmr_fk_min_height.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp]
    L.gmr_group_create.restype = vp
    L.gmr_group_create.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.gmr_group_destroy.argtypes = [vp]
    L.gmr_group_size.restype = C.c_int
    L.gmr_group_size.argtypes = [vp]
    L.gmr_group_model.restype = vp
    L.gmr_group_model.argtypes = [vp, C.c_int]
    L.gmr_group_last_error.restype = C.c_char_p
    L.gmr_group_last_error.argtypes = [vp]
    L.gmr_motion_epilogue.restype = C.c_int
    L.gmr_motion_epilogue.argtypes = [vp, C.POINTER(MotionInput), vp]
    L.gmr_group_motion_epilogue.restype = C.c_int
    L.gmr_group_motion_epilogue.argtypes = [vp, C.POINTER(MotionInput), vp]
    L.gmr_motion_track.restype = C.c_int
    L.gmr_motion_track.argtypes = [vp, C.POINTER(TrackInput), vp]
    L.gmr_group_motion_track.restype = C.c_int
    L.gmr_group_motion_track.argtypes = [vp, C.POINTER(TrackInput), vp]
    L.gmr_lowpass_coefficients.restype = C.c_int
    L.gmr_lowpass_coefficients.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double)]
    L.gmr_motion_sample.restype = C.c_int
    L.gmr_motion_sample.argtypes = [vp, C.POINTER(SampleInput), vp]
    L.gmr_motion_contacts.restype = C.c_int
    L.gmr_motion_contacts.argtypes = [vp, C.POINTER(ContactInput)]
    L.gmr_motion_footlock.restype = C.c_int
    L.gmr_motion_footlock.argtypes = [vp, C.POINTER(FootlockInput)]
    L.gmr_motion_dynamics.restype = C.c_int
    L.gmr_motion_dynamics.argtypes = [vp, C.POINTER(DynamicsInput)]
    L.gmr_motion_self_collision.restype = C.c_int
    L.gmr_motion_self_collision.argtypes = [vp, C.POINTER(SelfCollisionInput)]
    L.gmr_motion_self_collision_repair.restype = C.c_int
    L.gmr_motion_self_collision_repair.argtypes = [vp, C.POINTER(SelfCollisionRepairInput)]
    L.gmr_motion_mirror.restype = C.c_int
    L.gmr_motion_mirror.argtypes = [vp, C.POINTER(MirrorInput)]
    L.gmr_motion_compose.restype = C.c_int
    L.gmr_motion_compose.argtypes = [vp, C.POINTER(ComposeInput)]
    L.gmr_motion_transitions.restype = C.c_int
    L.gmr_motion_transitions.argtypes = [vp, C.POINTER(TransitionsInput)]
    L.gmr_motion_retime_plan.restype = C.c_int
    L.gmr_motion_retime_plan.argtypes = [vp, C.POINTER(RetimePlanInput)]
    L.gmr_motion_retime_apply.restype = C.c_int
    L.gmr_motion_retime_apply.argtypes = [vp, C.POINTER(RetimeApplyInput)]
    L.gmr_motion_retime_plan_torque.restype = C.c_int
    L.gmr_motion_retime_plan_torque.argtypes = [vp, C.POINTER(RetimeTorqueInput)]
    L.gmr_clip_report.restype = C.c_int
    L.gmr_clip_report.argtypes = [vp, C.POINTER(ClipReportInput), C.POINTER(ClipReportParams), vp]
    L.gmr_group_clip_report.restype = C.c_int
    L.gmr_group_clip_report.argtypes = [vp, C.POINTER(ClipReportInput), C.POINTER(ClipReportParams), vp]
    L.gmr_bvh_parse_header.restype = C.c_int
    L.gmr_bvh_parse_header.argtypes = [vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.gmr_evaluate.restype = C.c_int
    L.gmr_evaluate.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.gmr_smplx_keypoints.restype = C.c_int
    L.gmr_smplx_keypoints.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, C.c_int, vp, vp, vp]
    L.gmr_smplx_keypoints_cols.restype = C.c_int
    L.gmr_smplx_keypoints_cols.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int64, C.c_int, vp, C.c_int, vp, vp, vp]
    L.gmr_smplx_keypoints_in.restype = C.c_int
    L.gmr_smplx_keypoints_in.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int64, C.c_int64, C.c_int, vp, C.c_int, vp, vp, vp]
    L.gmr_smplx_body.restype = C.c_int
    L.gmr_smplx_body.argtypes = [vp, C.c_int, C.POINTER(SmplxBodyClip), C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    L.gmr_bvh_fk_rows.restype = C.c_int
    L.gmr_bvh_fk_rows.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int64, C.c_int64, C.c_double, vp, C.c_int, vp, vp, vp]
    L.gmr_bvh_parse_motion_device.restype = C.c_int
    L.gmr_bvh_parse_motion_device.argtypes = [vp, C.c_int64, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    L.gmr_bvh_fk.restype = C.c_int
    L.gmr_bvh_fk.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int64, C.c_double, vp, vp, vp]
    L.gmr_bvh_parse_motion.restype = C.c_int64
    L.gmr_bvh_parse_motion.argtypes = [vp, C.c_size_t, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.gmr_session_create.restype = vp
    L.gmr_session_create.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(IKParams)]
    L.gmr_session_destroy.argtypes = [vp]
    L.gmr_session_reset.restype = C.c_int
    L.gmr_session_reset.argtypes = [vp, vp]
    L.gmr_session_step.restype = C.c_int
    L.gmr_session_step.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    L.gmr_session_state.restype = C.c_int
    L.gmr_session_state.argtypes = [vp, vp]
    L.gmr_session_set_persistent.restype = C.c_int
    L.gmr_session_set_persistent.argtypes = [vp, C.c_int]
    _lib = L
    return L
