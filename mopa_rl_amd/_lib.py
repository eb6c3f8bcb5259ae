"""ctypes binding of libmopa_hip.so (the C ABI in include/mopa_hip.h).

There is no CPU fallback: if the shared library is missing, or no HIP device
is visible when a scene is created, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MOPA_HIP_LIB", os.path.join(_HERE, "csrc", "libmopa_hip.so"))   # env override: A/B builds

MOPA_OK = 0
MOPA_FAR = 1.0e10
PLAN_OK, PLAN_NO_EXACT, PLAN_INVALID_GOAL = 0, -4, -5

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

# every symbol include/mopa_hip.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "mopa_last_error", "mopa_version", "mopa_device_count", "mopa_scene_create", "mopa_scene_destroy",
    "mopa_scene_create_glued", "mopa_scene_glue", "mopa_glue_attach_batch", "mopa_glue_rows_batch", "mopa_scene_k1_export_glued",
    "mopa_scene_num_active", "mopa_scene_active_idx", "mopa_scene_num_pairs", "mopa_scene_lds_bytes", "mopa_scene_valid_kernel",
    "mopa_scene_motion_kernel",
    "mopa_scene_k1_baked", "mopa_scene_k1_drain_plan", "mopa_scene_k1_export", "mopa_scene_hdr_offset", "mopa_k1_baked_fk_host", "mopa_k1_baked_fk_sparse_host", "mopa_k1_baked_fk_pose_host", "mopa_k1_baked_resident_host", "mopa_k1_baked_static_host",
    "mopa_is_valid_batch", "mopa_is_valid_batch_counted", "mopa_check_motion_batch", "mopa_plan_batch", "mopa_simplify_paths_batch", "mopa_simplify_paths_max_path", "mopa_shortcut_paths_batch", "mopa_shortcut_paths_max_path", "mopa_smooth_paths_batch", "mopa_smooth_paths_max_path",
    "mopa_plan_star_batch", "mopa_plan_star", "mopa_plan_star_k", "mopa_star_params_size",
    "mopa_plan_star_clearance_batch", "mopa_plan_star_clearance",
    "mopa_plan_race_batch", "mopa_plan_race", "mopa_race_params_size", "mopa_pullback_batch", "mopa_is_valid_state", "mopa_plan",
    "mopa_planner_status", "mopa_debug_fk", "mopa_debug_pair_dist", "mopa_contacts_batch", "mopa_contacts_state",
    "mopa_contact_frames_batch", "mopa_contact_frames_state", "mopa_geom_frames_batch", "mopa_geom_frames_host",
    "mopa_contact_manifolds_batch", "mopa_contact_manifolds_state", "mopa_geom_manifolds_batch", "mopa_geom_manifolds_host",
    "mopa_proximity_batch", "mopa_proximity_state", "mopa_geom_sep_batch", "mopa_geom_sep_host",
    "mopa_proximity_exact_batch", "mopa_proximity_exact_state", "mopa_geom_sep_exact_batch", "mopa_geom_sep_exact_host",
    "mopa_proximity_witness_batch", "mopa_proximity_witness_state", "mopa_geom_witness_batch", "mopa_geom_witness_host",
    "mopa_motion_clearance_exact_batch", "mopa_motion_clearance_exact",
    "mopa_motion_report_batch", "mopa_motion_report", "mopa_motion_clearance_batch", "mopa_motion_clearance",
    "mopa_env_create", "mopa_env_destroy", "mopa_env_obs_dim", "mopa_env_action_dim", "mopa_env_step_batch", "mopa_env_exec_batch", "mopa_env_desired_batch",
    "mopa_env_attach_dynamics", "mopa_env_attach_contacts", "mopa_env_set_contact_stats", "mopa_rollout_stage", "mopa_rollout_pool_pick", "mopa_rollout_step_size", "mopa_reuse_batch", "mopa_replay_append", "mopa_replay_sample", "mopa_ct_desc_size", "mopa_env_contact_arena", "mopa_env_dyn_dofs", "mopa_env_dyn_qvel_width", "mopa_env_dyn_waves", "mopa_env_dyn_forward_batch", "mopa_env_dyn_substeps_batch", "mopa_env_step_dyn_batch",
    "mopa_pusher_dyn_desc_size", "mopa_env_attach_pusher_dynamics", "mopa_env_set_pusher_stats", "mopa_env_pusher_substeps_batch",
    "mopa_env_step_pusher_batch", "mopa_env_set_contact_force",
    "mopa_ik_create", "mopa_ik_destroy", "mopa_ik_solve_batch", "mopa_ik_site_pose_batch", "mopa_ik_targets_batch",
    "mopa_ik_targets_pos_batch", "mopa_ik_displacement_pos_batch",
    "mopa_env_tables_host", "mopa_ik_tables_host", "mopa_dyn_tables_host",
    "mopa_paths_unwrap_batch", "mopa_paths_unwrap_seam_batch", "mopa_paths_walk_batch", "mopa_paths_assemble_batch", "mopa_interpolate_batch",
]


class MopaError(RuntimeError):
    pass


class MopaModel(C.Structure):
    _fields_ = [
        ("nq", C.c_int32), ("nbody", C.c_int32), ("njnt", C.c_int32), ("ngeom", C.c_int32), ("npair", C.c_int32),
        ("body_parent", _ip), ("body_pos", _dp), ("body_quat", _dp), ("body_jntadr", _ip), ("body_jntnum", _ip),
        ("jnt_type", _ip), ("jnt_qposadr", _ip), ("jnt_axis", _dp), ("jnt_pos", _dp), ("jnt_ref", _dp),
        ("jnt_limited", _ip), ("jnt_range", _dp),
        ("geom_type", _ip), ("geom_body", _ip), ("geom_mjid", _ip), ("geom_size", _dp), ("geom_pos", _dp),
        ("geom_quat", _dp), ("pair_geom", _ip),
        ("nmesh", C.c_int32), ("nmeshvert", C.c_int32), ("mesh_vertadr", _ip), ("mesh_vertnum", _ip), ("mesh_vert", _dp),
        ("geom_dataid", _ip),
    ]


class MopaSceneDesc(C.Structure):
    _fields_ = [
        ("model", MopaModel), ("n_passive", C.c_int32), ("passive_qpos_idx", _ip), ("n_ignored", C.c_int32),
        ("ignored_pairs", _ip), ("contact_threshold", C.c_double), ("range", C.c_double), ("resolution", C.c_double),
        ("seed", C.c_uint64), ("device", C.c_int32), ("pair_cull_radius", _dp),
    ]


class MopaEnvDesc(C.Structure):
    _fields_ = [
        ("model", MopaModel), ("kind", C.c_int32), ("n_arm", C.c_int32), ("arm_qpos_idx", _ip), ("n_grip", C.c_int32), ("grip_qpos_idx", _ip),
        ("n_act", C.c_int32), ("act_qpos_idx", _ip), ("act_ctrl_lo", _dp), ("act_ctrl_hi", _dp),
        ("n_frames", C.c_int32), ("frame_body", _ip), ("frame_off", _dp), ("n_quats", C.c_int32), ("quat_body", _ip),
        ("n_touch", C.c_int32), ("touch_geom", _ip), ("n_touch_left", C.c_int32),
        ("qpos_min", _dp), ("qpos_max", _dp), ("qpos_limited", _ip),
        ("ac_scale", C.c_double), ("distance_threshold", C.c_double), ("success_reward", C.c_double),
        ("max_episode_steps", C.c_int32), ("device", C.c_int32),
    ]


class MopaObjDesc(C.Structure):
    _fields_ = [
        ("qadr", C.c_int32), ("mass", C.c_double), ("inertia", C.c_double * 3), ("damping", C.c_double),
        ("half", C.c_double * 3), ("rbound", C.c_double), ("nfeat", C.c_int32), ("feat", _dp),
        ("ncol", C.c_int32), ("co_body", _ip), ("co_type", _ip), ("co_size", _dp), ("co_pos", _dp), ("co_mat", _dp),
        ("co_mu", _dp), ("co_rbound", _dp), ("inv_mass", C.c_double), ("inv_inertia", C.c_double * 3),
        ("precull_every", C.c_int32), ("precull_margin", C.c_double),
        ("kn", C.c_double), ("dn", C.c_double), ("eps_v", C.c_double), ("ct_max", C.c_double),
    ]


class MopaDynDesc(C.Structure):
    _fields_ = [
        ("nd", C.c_int32), ("parent", _ip), ("jtype", _ip), ("qadr", _ip), ("rel_pos", _dp), ("rel_quat", _dp),
        ("axis", _dp), ("jpos", _dp), ("qref", _dp), ("mass", _dp), ("ipos", _dp), ("inertia", _dp),
        ("damping", _dp), ("armature", _dp), ("limited", _ip), ("lo", _dp), ("hi", _dp),
        ("actuated", _ip), ("kp", _dp), ("force_lo", _dp), ("force_hi", _dp), ("gravcomp", _ip),
        ("gravity", C.c_double * 3), ("timestep", C.c_double), ("nsub", C.c_int32), ("obj", C.POINTER(MopaObjDesc)),
    ]


class MopaRolloutStep(C.Structure):
    """include/mopa_hip.h MopaRolloutStep: every pointer as an address (c_void_p), filled from tensors' data_ptr()"""
    _I32 = ("nq", "n_arm", "ac_dim", "ac_stride", "adim", "obs_dim", "K", "discrete", "normal_space")
    _F64 = ("omega", "ac_scale", "action_range", "omega_over_scale", "one_minus_omega", "range_minus_scale")
    _PTR = ("lim_lo", "lim_hi", "lo_state", "hi_state", "lo_shrunk", "hi_shrunk", "safe_q",
            "qpos", "obs", "reward", "done", "success", "has_prev",
            "busy", "pool_mask", "interp_overflow", "wait_since", "t_dev", "t_env", "pend_type", "q_cur", "q_tgt", "pend_ob", "pend_ac",
            "c_rl", "c_interp", "c_mp_fail", "c_invalid",
            "ac", "ac_type_in", "a_in",
            "prev_ob", "ac_tr", "a", "extra_ac", "target", "cur_m", "cur_v", "tgt_v", "traj",
            "active", "is_pl", "pv", "plan_ok", "ac_type", "path_len", "tv", "ok", "nst", "tlen", "finished",
            "act0", "flags", "sitting", "stepped", "is_pl_out", "plen_m", "last_extra", "rew", "done_out", "intra", "ob_next", "success_out", "retry_mask", "pool_counts")
    _fields_ = ([("E", C.c_int64)] + [(k, C.c_int32) for k in _I32] + [(k, C.c_double) for k in _F64] + [(k, C.c_void_p) for k in _PTR])


class MopaCtDesc(C.Structure):
    _fields_ = [
        ("ns", C.c_int32), ("sh_body", _ip), ("sh_type", _ip), ("sh_size", _dp), ("sh_pos", _dp), ("sh_mat", _dp), ("sh_rbound", _dp),
        ("sh_feat0", _ip), ("nf", C.c_int32), ("ft_pos", _dp), ("ft_rad", _dp),
        ("np", C.c_int32), ("pr_f", _ip), ("pr_s", _ip), ("pr_par", _dp),
        ("obj_qadr", C.c_int32), ("obj_mass", C.c_double), ("obj_inertia", C.c_double * 3), ("obj_ipos", C.c_double * 3),
        ("obj_iquat", C.c_double * 4), ("obj_damping", C.c_double), ("obj_inv_mass", C.c_double), ("obj_inv_inertia", C.c_double * 3),
        ("obj_inv_mass_d", C.c_double), ("obj_inv_inertia_d", C.c_double * 3),
        ("maxcon", C.c_int32), ("maxpair", C.c_int32), ("iterations", C.c_int32), ("tolerance", C.c_double), ("inv_scale", C.c_double),
        ("precull_every", C.c_int32), ("precull_margin", C.c_double), ("near_every", C.c_int32), ("near_margin", C.c_double), ("warmstart", C.c_int32),
        ("solver", C.c_int32), ("limit_rows", C.c_int32), ("lim_par", C.c_double * 8), ("noslip_iterations", C.c_int32), ("noslip_tolerance", C.c_double),
        ("arena", C.c_int32),
    ]


class MopaPusherDynDesc(C.Structure):
    _fields_ = [
        ("qadr", C.c_int32 * 6), ("limited", C.c_int32 * 6), ("lo", C.c_double * 6), ("hi", C.c_double * 6),
        ("armature", C.c_double * 6), ("damping", C.c_double * 6), ("base", C.c_double * 2), ("rel", C.c_double * 8),
        ("mass", C.c_double * 4), ("com", C.c_double * 8), ("izz", C.c_double * 4),
        ("box_mass", C.c_double), ("box_org", C.c_double * 2), ("box_ref", C.c_double * 2),
        ("gear", C.c_double * 4), ("kv", C.c_double * 4), ("ctrl_lo", C.c_double * 4), ("ctrl_hi", C.c_double * 4),
        ("kp", C.c_double), ("kd", C.c_double), ("ki", C.c_double), ("alpha", C.c_double),
        ("frame_dt", C.c_double), ("timestep", C.c_double), ("nsub", C.c_int32), ("iterations", C.c_int32),
        ("tolerance", C.c_double), ("inv_scale", C.c_double), ("lim_par", C.c_double * 8),
        ("maxcon", C.c_int32), ("npair", C.c_int32), ("pairs", _dp),
    ]


class MopaIkDesc(C.Structure):
    _fields_ = [("model", MopaModel), ("n_joints", C.c_int32), ("joint_ids", _ip), ("site_body", C.c_int32),
                ("site_off", C.c_double * 3), ("site_quat", C.c_double * 4), ("device", C.c_int32)]


class MopaPlanParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("max_nodes", C.c_int32), ("max_path", C.c_int32), ("seed", C.c_uint64),
                ("env_id_base", C.c_uint64), ("env_ids_dev", C.c_void_p), ("seeds_dev", C.c_void_p), ("max_workgroups", C.c_int32), ("exclusive_cu", C.c_int32),
                ("tree_q_dev", C.c_void_p), ("tree_p_dev", C.c_void_p), ("state_dev", C.c_void_p),
                ("resume_tree_q", C.c_void_p), ("resume_tree_p", C.c_void_p), ("resume_state", C.c_void_p)]


class MopaStarParams(C.Structure):
    """include/mopa_hip.h MopaStarParams (K3b RRT*)"""
    _fields_ = [("max_iters", C.c_int32), ("max_nodes", C.c_int32), ("max_path", C.c_int32), ("seed", C.c_uint64),
                ("env_id_base", C.c_uint64), ("env_ids_dev", C.c_void_p), ("seeds_dev", C.c_void_p), ("goal_bias", C.c_double),
                ("goal_threshold", C.c_double), ("rewire_factor", C.c_double), ("max_workgroups", C.c_int32)]


class MopaRaceParams(C.Structure):
    """include/mopa_hip.h MopaRaceParams (K3 race: `portfolio` seeded RRT-Connect members per query)"""
    _fields_ = [("max_iters", C.c_int32), ("max_nodes", C.c_int32), ("max_path", C.c_int32), ("portfolio", C.c_int32), ("seed", C.c_uint64),
                ("env_id_base", C.c_uint64), ("env_ids_dev", C.c_void_p), ("seeds_dev", C.c_void_p), ("max_workgroups", C.c_int32),
                ("no_abort", C.c_int32)]


RACE_INFO_COLS = 3          # members cut, checks spent by all members, the winner's iterations (-1: none)
RACE_SEED_STEP = 0x9E3779B97F4A7C15     # member m of a query runs the seed (seed + m * RACE_SEED_STEP) mod 2^64
STAR_INFO_COLS = 8          # iterations run, nodes, motion checks, rewires, goal nodes, first goal iteration, descendant updates, full-tree iterations
STAR_CLEARANCE_INFO_COLS = 11   # ... with motion evaluations in column 2, then parent-walk evaluations, rewire evaluations, rewires that raised the clearance
STAR_REWIRE_FACTOR = 1.1    # OMPL's default
STAR_GOAL_BIAS = 0.05       # OMPL's default

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libmopa_hip.so (built in-tree by __graft_entry__.build / csrc/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MopaError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C mopa_rl_amd/csrc`). There is no CPU fallback.")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 and must be loaded first so
    # that libmopa_hip.so binds to that same copy (two runtimes in one process cannot both own the GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.mopa_last_error.restype = C.c_char_p
    L.mopa_version.restype = C.c_char_p
    L.mopa_device_count.restype = C.c_int
    L.mopa_scene_create.argtypes = [C.POINTER(MopaSceneDesc), C.POINTER(vp)]
    L.mopa_scene_destroy.argtypes = [vp]
    L.mopa_scene_destroy.restype = None
    L.mopa_scene_create_glued.argtypes = [C.POINTER(MopaSceneDesc), C.c_int32, C.c_int32, C.POINTER(vp)]
    L.mopa_scene_glue.argtypes = [vp, _ip]
    L.mopa_glue_attach_batch.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.mopa_glue_rows_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, vp]
    L.mopa_scene_k1_export_glued.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.mopa_scene_num_active.argtypes = [vp]
    L.mopa_scene_active_idx.argtypes = [vp, _ip]
    L.mopa_scene_num_pairs.argtypes = [vp]
    L.mopa_scene_lds_bytes.argtypes = [vp]
    L.mopa_is_valid_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.mopa_is_valid_batch_counted.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp]
    L.mopa_check_motion_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int64, vp, vp]
    L.mopa_plan_batch.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(MopaPlanParams), vp, vp, vp, vp, vp]
    L.mopa_simplify_paths_batch.argtypes = [vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int32, vp, vp]
    L.mopa_simplify_paths_max_path.argtypes = [vp]
    L.mopa_shortcut_paths_batch.argtypes = [vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int32, C.c_int32, vp, vp]
    L.mopa_shortcut_paths_max_path.argtypes = [vp]
    L.mopa_smooth_paths_batch.argtypes = [vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, C.c_int32, C.c_int32, vp, vp]
    L.mopa_smooth_paths_max_path.argtypes = [vp]
    L.mopa_plan_star_batch.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(MopaStarParams), vp, vp, vp, vp, vp, vp]
    L.mopa_plan_star.argtypes = [vp, _dp, _dp, C.POINTER(MopaStarParams), _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.mopa_plan_star_k.argtypes = [C.c_int32, C.c_int64, C.c_double]
    L.mopa_plan_star_clearance_batch.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(MopaStarParams), C.c_double, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_plan_star_clearance.argtypes = [vp, _dp, _dp, C.POINTER(MopaStarParams), C.c_double, _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.mopa_star_params_size.argtypes = []
    L.mopa_plan_race_batch.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(MopaRaceParams), vp, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_plan_race.argtypes = [vp, _dp, _dp, C.POINTER(MopaRaceParams), _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
    L.mopa_race_params_size.argtypes = []
    L.mopa_pullback_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_double, C.c_int32, vp, vp, vp]
    L.mopa_is_valid_state.argtypes = [vp, _dp, C.POINTER(C.c_int32), _dp]
    L.mopa_plan.argtypes = [vp, _dp, _dp, C.POINTER(MopaPlanParams), _dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                            C.POINTER(C.c_int64)]
    L.mopa_planner_status.argtypes = [vp]
    L.mopa_planner_status.restype = C.c_char_p
    L.mopa_debug_fk.argtypes = [vp, _dp, _dp, _dp]
    L.mopa_debug_pair_dist.argtypes = [vp, _dp, _dp]
    L.mopa_contacts_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_double, C.c_int32, vp, vp, vp, vp]
    L.mopa_contacts_state.argtypes = [vp, _dp, C.c_double, C.c_int32, _ip, _ip, _dp]
    L.mopa_contact_frames_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_double, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.mopa_contact_frames_state.argtypes = [vp, _dp, C.c_double, C.c_int32, _ip, _ip, _dp, _dp, _dp]
    L.mopa_geom_frames_batch.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, vp]
    L.mopa_geom_frames_host.argtypes = [C.c_int64, _ip, _dp, _dp, C.c_int32, _dp]
    L.mopa_contact_manifolds_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_contact_manifolds_state.argtypes = [vp, _dp, C.c_double, C.c_double, C.c_int32, C.c_int32, _ip, _ip, _dp, _dp, _ip, _dp, _dp]
    L.mopa_geom_manifolds_batch.argtypes = [C.c_int32, C.c_int64, vp, vp, C.c_double, C.c_int32, vp, vp, vp, vp]
    L.mopa_geom_manifolds_host.argtypes = [C.c_int64, _ip, _dp, _dp, C.c_int32, C.c_double, C.c_int32, _dp, _ip, _dp]
    L.mopa_proximity_batch.argtypes = [vp, vp, vp, C.c_int64, C.c_int64, C.c_double, C.c_int32, vp, vp, vp, vp, vp]
    L.mopa_proximity_state.argtypes = [vp, _dp, C.c_double, C.c_int32, _dp, _ip, _ip, _dp]
    L.mopa_geom_sep_batch.argtypes = [C.c_int32, C.c_int64, vp, vp, vp, C.c_int32, C.c_double, vp, vp]
    L.mopa_geom_sep_host.argtypes = [C.c_int64, _ip, _dp, _dp, C.c_int32, C.c_double, _dp]
    L.mopa_proximity_exact_batch.argtypes = L.mopa_proximity_batch.argtypes
    L.mopa_proximity_exact_state.argtypes = L.mopa_proximity_state.argtypes
    L.mopa_geom_sep_exact_batch.argtypes = L.mopa_geom_sep_batch.argtypes
    L.mopa_geom_sep_exact_host.argtypes = [C.c_int64, _ip, _dp, _dp, C.c_int32, C.c_double, _dp, _ip]
    L.mopa_proximity_witness_batch.argtypes = L.mopa_proximity_batch.argtypes[:-1] + [vp, vp, vp, vp]
    L.mopa_proximity_witness_state.argtypes = L.mopa_proximity_state.argtypes + [_dp, _dp, _dp]
    L.mopa_geom_witness_batch.argtypes = L.mopa_geom_sep_batch.argtypes
    L.mopa_geom_witness_host.argtypes = L.mopa_geom_sep_exact_host.argtypes
    L.mopa_motion_report_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp]
    L.mopa_motion_report.argtypes = [vp, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp, C.c_int32, _ip, _ip, _dp]
    L.mopa_motion_clearance_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_motion_clearance.argtypes = [vp, _dp, _dp, C.c_double, _dp, _ip, _ip, _ip, _dp, _ip, _dp, _dp]
    L.mopa_motion_clearance_exact_batch.argtypes = L.mopa_motion_clearance_batch.argtypes
    L.mopa_motion_clearance_exact.argtypes = L.mopa_motion_clearance.argtypes
    L.mopa_env_create.argtypes = [C.POINTER(MopaEnvDesc), C.POINTER(vp)]
    L.mopa_env_destroy.argtypes = [vp]
    L.mopa_env_destroy.restype = None
    L.mopa_env_step_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.mopa_env_obs_dim.argtypes = [vp]
    L.mopa_env_action_dim.argtypes = [vp]
    L.mopa_env_exec_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_env_desired_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, C.c_int32, vp, vp]
    L.mopa_env_attach_dynamics.argtypes = [vp, C.POINTER(MopaDynDesc)]
    L.mopa_env_attach_contacts.argtypes = [vp, C.POINTER(MopaCtDesc)]
    L.mopa_env_set_contact_stats.argtypes = [vp, vp]
    L.mopa_rollout_stage.argtypes = [C.POINTER(MopaRolloutStep), C.c_int32, vp]
    L.mopa_rollout_pool_pick.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_int64] + [vp] * 4 + [C.c_int64] + [vp] * 7
    L.mopa_rollout_step_size.argtypes = []
    L.mopa_reuse_batch.argtypes = ([C.c_int64] + [C.c_int32] * 6 + [vp] * 7 + [C.c_double] * 6 + [C.c_int32, vp, C.c_int32, vp, C.c_uint64, C.c_int64, C.c_int64,
                                                                                                   C.c_int64] + [vp] * 13)
    L.mopa_replay_append.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, C.c_int64, vp, vp, vp, vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.mopa_replay_sample.argtypes = [C.c_int64, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, vp]
    L.mopa_ct_desc_size.argtypes = []
    L.mopa_env_contact_arena.argtypes = [vp]
    L.mopa_env_contact_arena.restype = C.c_int
    L.mopa_env_dyn_dofs.argtypes = [vp]
    L.mopa_env_dyn_qvel_width.argtypes = [vp]
    L.mopa_env_dyn_waves.argtypes = [vp]
    L.mopa_env_dyn_forward_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mopa_env_dyn_substeps_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, C.c_int32, vp]
    L.mopa_env_step_dyn_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.mopa_pusher_dyn_desc_size.argtypes = []
    L.mopa_env_attach_pusher_dynamics.argtypes = [vp, C.POINTER(MopaPusherDynDesc)]
    L.mopa_env_set_pusher_stats.argtypes = [vp, vp]
    L.mopa_env_pusher_substeps_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int32, vp]
    L.mopa_env_step_pusher_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.mopa_env_set_contact_force.argtypes = [vp, vp, vp, vp, vp, C.c_int32]
    L.mopa_ik_create.argtypes = [C.POINTER(MopaIkDesc), C.POINTER(vp)]
    # host halves of env / IK / dynamics creation (no device): status code, fingerprint of the tables, table counts
    u64p = C.POINTER(C.c_uint64)
    L.mopa_env_tables_host.argtypes = [C.POINTER(MopaEnvDesc), u64p, _ip, _ip]
    L.mopa_ik_tables_host.argtypes = [C.POINTER(MopaIkDesc), u64p, _ip]
    L.mopa_dyn_tables_host.argtypes = [C.POINTER(MopaEnvDesc), C.POINTER(MopaDynDesc), u64p, _ip]
    L.mopa_ik_destroy.argtypes = [vp]
    L.mopa_ik_destroy.restype = None
    L.mopa_ik_solve_batch.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                      vp, vp, vp, vp]
    L.mopa_ik_site_pose_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    L.mopa_ik_targets_batch.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, vp, vp]
    L.mopa_ik_targets_pos_batch.argtypes = [vp, C.c_int64, vp, vp, C.c_int64, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, vp]
    L.mopa_ik_displacement_pos_batch.argtypes = [vp, C.c_int64, vp, vp, C.c_int64, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                 C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_scene_valid_kernel.argtypes = [vp, C.c_int64, C.c_char_p, C.c_int32]
    L.mopa_scene_motion_kernel.argtypes = [vp, C.c_int64, C.c_char_p, C.c_int32]
    L.mopa_scene_k1_baked.argtypes = [vp]
    L.mopa_scene_k1_drain_plan.argtypes = [vp, C.c_int64, C.c_int32, _ip, _ip]
    L.mopa_scene_k1_export.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.mopa_scene_hdr_offset.argtypes = [C.c_char_p]
    L.mopa_k1_baked_fk_host.argtypes = [C.c_int, C.c_int64, vp, vp, vp]
    L.mopa_k1_baked_fk_sparse_host.argtypes = [C.c_int, C.c_int64, vp, vp, vp, vp]
    L.mopa_k1_baked_fk_pose_host.argtypes = [C.c_int, C.c_int64, vp, vp, vp]
    L.mopa_k1_baked_resident_host.argtypes = [C.c_int, C.c_int64, vp, vp, vp, vp]
    L.mopa_k1_baked_static_host.argtypes = [C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp]
    i32, i64, f64 = C.c_int32, C.c_int64, C.c_double
    L.mopa_paths_unwrap_batch.argtypes = [C.c_int, i64, i32, i32, vp, i32, vp, vp, vp, f64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_paths_unwrap_seam_batch.argtypes = [C.c_int, i64, i32, i32, vp, i32, vp, vp, vp, f64, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, vp]
    L.mopa_paths_walk_batch.argtypes = [C.c_int, i64, i32, i32, vp, i32, vp, vp, f64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mopa_paths_assemble_batch.argtypes = [C.c_int, i64, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    L.mopa_interpolate_batch.argtypes = [vp, i64, i32, i32, vp, vp, f64, vp, vp, vp, vp, vp]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != MOPA_OK:
        raise MopaError(f"libmopa_hip error {rc}: {lib().mopa_last_error().decode()}")


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _pair_names(model, pair, dist, n):
    """the first min(n, len(pair)) records of a report row as (geom1_name, geom2_name, dist), `pair` indexing `model.pair_geom`"""
    g = np.asarray(model.pair_geom).reshape(-1, 2)
    name = lambda k: model.all_geom_names[int(model.geom_mjid[int(k)])]
    k = min(int(n), len(pair))
    return [(name(g[p, 0]), name(g[p, 1]), float(d)) for p, d in zip(pair[:k], dist[:k])]


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def geom_frames_host(types, recs, mesh_verts=None) -> np.ndarray:
    """mopa_geom_frames_host: M posed pairs -- types [M, 2] (MuJoCo geom type codes, either order), recs [M, 2, 15] = pos[3]
    mat[9] size[3] per geom -> [M, 7] = dist, normal[3], pos[3] by the host compile of the kernels' functions (no GPU).
    mesh_verts [n, 3]: the hull of the mesh that every pair with a second geom of type 7 has."""
    t, tp = _i(np.asarray(types).reshape(-1, 2))
    r, rp = _d(np.asarray(recs, dtype=np.float64).reshape(-1, 30))
    if len(t) != len(r):
        raise MopaError(f"{len(t)} type pairs for {len(r)} record pairs")
    out = np.zeros((len(t), 7))
    v, vp_ = _d(np.asarray(mesh_verts, dtype=np.float64).reshape(-1, 3)) if mesh_verts is not None else (np.zeros((0, 3)), None)
    check(lib().mopa_geom_frames_host(len(t), tp, rp, vp_, len(v), out.ctypes.data_as(_dp)))
    return out


def geom_manifolds_host(types, recs, mesh_verts=None, point_cutoff: float = 0.0, max_points: int = 4):
    """mopa_geom_manifolds_host: M posed pairs as `geom_frames_host` takes them -> (normal_dist [M, 4] = normal[3], dist;
    npoint [M] int32; points [M, P, 4] = pos[3], dist_i) by the host compile of the kernels' geom_manifold (no GPU): the frame's
    normal and up to P = max_points contact points under point_cutoff, deepest first; MOPA_FAR / 0.0 in unused point slots
    ("Contact manifolds"; PARITY UNPINNED)."""
    t, tp = _i(np.asarray(types).reshape(-1, 2))
    r, rp = _d(np.asarray(recs, dtype=np.float64).reshape(-1, 30))
    if len(t) != len(r):
        raise MopaError(f"{len(t)} type pairs for {len(r)} record pairs")
    P = int(max_points)
    nd = np.zeros((len(t), 4))
    npoint = np.zeros(len(t), dtype=np.int32)
    pts = np.zeros((len(t), max(P, 1), 4))
    v, vp_ = _d(np.asarray(mesh_verts, dtype=np.float64).reshape(-1, 3)) if mesh_verts is not None else (np.zeros((0, 3)), None)
    check(lib().mopa_geom_manifolds_host(len(t), tp, rp, vp_, len(v), float(point_cutoff), P, nd.ctypes.data_as(_dp), npoint.ctypes.data_as(_ip),
                                         pts.ctypes.data_as(_dp)))
    return nd, npoint, pts


def geom_sep_host(types, recs, band: float, mesh_verts=None, exact: bool = False, return_iters: bool = False):
    """mopa_geom_sep_host: M posed pairs as `geom_frames_host` takes them -> [M] band-limited signed distances by the host compile
    of the kernels' geom_sep (no GPU): d where d <= band, MOPA_FAR otherwise ("Proximity report").
    exact=True (mopa_geom_sep_exact_host): disjoint box-box, cylinder and mesh pairs get the GJK distance, at most 1e-6 above the
    true one, instead of the margin rule's.  return_iters=True (with exact=True): -> (out, iters [M] int32), the exact route's
    number of support evaluations per pair, 0 where it was not taken, negative where its iteration cap ended it."""
    if return_iters and not exact:
        raise MopaError("return_iters needs exact=True")
    t, tp = _i(np.asarray(types).reshape(-1, 2))
    r, rp = _d(np.asarray(recs, dtype=np.float64).reshape(-1, 30))
    if len(t) != len(r):
        raise MopaError(f"{len(t)} type pairs for {len(r)} record pairs")
    out = np.zeros(len(t))
    v, vp_ = _d(np.asarray(mesh_verts, dtype=np.float64).reshape(-1, 3)) if mesh_verts is not None else (np.zeros((0, 3)), None)
    if exact:
        iters = np.zeros(len(t), dtype=np.int32)
        check(lib().mopa_geom_sep_exact_host(len(t), tp, rp, vp_, len(v), float(band), out.ctypes.data_as(_dp), iters.ctypes.data_as(_ip)))
        return (out, iters) if return_iters else out
    check(lib().mopa_geom_sep_host(len(t), tp, rp, vp_, len(v), float(band), out.ctypes.data_as(_dp)))
    return out


def geom_witness_host(types, recs, band: float, mesh_verts=None, return_iters: bool = False):
    """mopa_geom_witness_host: M posed pairs as `geom_frames_host` takes them -> [M, 10] = d, n[3], p1[3], p2[3] by the host compile
    of the kernels' geom_witness (no GPU): d the bits of `geom_sep_host(..., exact=True)`; p1 a point of the first geom given, p2 of
    the second, with |p2 - p1| = d where the shapes are apart (to 1e-6 for box-box, cylinder and mesh pairs) and the contact
    frame's witness points pos -/+ (d / 2) n where they overlap; n the unit vector from the first geom towards the second.  The nine
    are 0.0 where d is MOPA_FAR ("Witness points").  return_iters=True: -> (out, iters [M] int32) as
    `geom_sep_host` returns them."""
    t, tp = _i(np.asarray(types).reshape(-1, 2))
    r, rp = _d(np.asarray(recs, dtype=np.float64).reshape(-1, 30))
    if len(t) != len(r):
        raise MopaError(f"{len(t)} type pairs for {len(r)} record pairs")
    out = np.zeros((len(t), 10))
    iters = np.zeros(len(t), dtype=np.int32)
    v, vp_ = _d(np.asarray(mesh_verts, dtype=np.float64).reshape(-1, 3)) if mesh_verts is not None else (np.zeros((0, 3)), None)
    check(lib().mopa_geom_witness_host(len(t), tp, rp, vp_, len(v), float(band), out.ctypes.data_as(_dp), iters.ctypes.data_as(_ip)))
    return (out, iters) if return_iters else out


def model_struct(m, keep: list, pair_geom=None) -> MopaModel:
    """MopaModel view of a CompiledModel; the numpy buffers it points at are appended to `keep`.
    pair_geom: a (reduced) candidate-pair list to hand over instead of the model's."""
    def d(a):
        a, p = _d(a); keep.append(a); return p

    def i(a):
        a, p = _i(a); keep.append(a); return p

    pairs = m.pair_geom if pair_geom is None else pair_geom
    return MopaModel(
        m.nq, len(m.body_names), len(m.jnt_names), len(m.geom_type), len(pairs),
        i(m.body_parent), d(m.body_pos), d(m.body_quat), i(m.body_jntadr), i(m.body_jntnum),
        i(m.jnt_type), i(m.jnt_qposadr), d(m.jnt_axis), d(m.jnt_pos), d(m.jnt_ref), i(m.jnt_limited), d(m.jnt_range),
        i(m.geom_type), i(m.geom_body), i(m.geom_mjid), d(m.geom_size), d(m.geom_pos), d(m.geom_quat), i(pairs),
        len(m.mesh_vertnum), len(m.mesh_vert), i(m.mesh_vertadr), i(m.mesh_vertnum), d(m.mesh_vert), i(m.geom_dataid))


def glue_ids(model, body_a, body_b):
    """(body_a, body_b) of a glue_bodies pair as model body ids; names (str / bytes) or ids"""
    def one(b):
        if isinstance(b, (bytes, bytearray)):
            b = b.decode("utf-8")
        if isinstance(b, str):
            names = list(model.body_names)
            if b not in names:
                raise MopaError(f"glue_bodies: the model has no body named {b!r}")
            return names.index(b)
        return int(b)
    return one(body_a), one(body_b)


def glue_subtree_geoms(model, body_b: int) -> np.ndarray:
    """bool per collidable geom: it sits on body_b or on a body below it"""
    par = np.asarray(model.body_parent)
    sub = np.zeros(len(par), dtype=bool)
    if 0 < body_b < len(par):
        sub[body_b] = True
        for b in range(body_b + 1, len(par)):
            sub[b] = sub[par[b]]
    return sub[np.asarray(model.geom_body)]


def scene_desc(model, passive_joint_idx, ignored_contacts, contact_threshold: float, range_: float = 0.1, resolution: float = 0.005,
               seed: int = 0, device: int = -1, prune_pairs: Optional[bool] = None, glue=None):
    """The MopaSceneDesc that Scene hands to mopa_scene_create (pair pruning and per-pair cull radii applied as described
    there) + the numpy buffers it points at + (pairs pruned, pairs with a tightened cull radius).
    glue = (body_a, body_b) ids: the description of the glued scene -- the pruning proofs were made with the object where the env row
    puts it, so every candidate pair with a geom on body_b or below it is kept, with no tightened cull radius."""
    m = model
    keep = []
    carried = glue_subtree_geoms(m, int(glue[1])) if glue is not None else np.zeros(len(m.geom_type), dtype=bool)
    if prune_pairs is None:
        prune_pairs = os.environ.get("MOPA_PRUNE_PAIRS", "1") != "0"
    pairs = np.asarray(m.pair_geom, dtype=np.int32).reshape(-1, 2)
    meta = getattr(m, "meta", {})
    never = list(meta.get("never_violating_pairs") or [])
    at = meta.get("never_violating_pairs_thr") or {}
    if at and float(contact_threshold) <= float(at.get("threshold", -np.inf)):
        never += list(at.get("pairs") or [])      # may touch, never reach a threshold this negative
    npair_pruned = 0
    if prune_pairs and len(never) and float(contact_threshold) <= 0.0:
        drop = {(int(a), int(b)) for a, b in never} | {(int(b), int(a)) for a, b in never}
        keep_row = np.array([(int(a), int(b)) not in drop or bool(carried[a] or carried[b]) for a, b in pairs], dtype=bool)
        npair_pruned = int((~keep_row).sum())
        pairs = np.ascontiguousarray(pairs[keep_row])

    def d(a):
        a, p = _d(a); keep.append(a); return p

    def i(a):
        a, p = _i(a); keep.append(a); return p

    ign = np.asarray(list(ignored_contacts), dtype=np.int32).reshape(-1, 2)
    pas = np.asarray(list(passive_joint_idx), dtype=np.int32)
    desc = MopaSceneDesc()
    desc.model = model_struct(m, keep, pair_geom=pairs)
    # per-pair bound on the centre distance at which the pair can reach the threshold (same proof machinery): the FP32
    # broad phase culls with it instead of the bounding-sphere sum (closed gripper fingers: 9 mm instead of 10 cm)
    cr = meta.get("pair_cull_radius") or {}
    npair_tightened = 0
    if prune_pairs and cr and float(contact_threshold) <= float(cr.get("threshold", -np.inf)):
        rad = {(int(a), int(b)): float(r) for a, b, r in cr.get("pairs") or []}
        arr = np.array([0.0 if (carried[a] or carried[b]) else rad.get((int(a), int(b)), rad.get((int(b), int(a)), 0.0)) for a, b in pairs],
                       dtype=np.float64)
        if (arr > 0).any():
            npair_tightened = int((arr > 0).sum())
            desc.pair_cull_radius = d(arr)
    desc.n_passive = len(pas)
    desc.passive_qpos_idx = i(pas)
    desc.n_ignored = len(ign)
    desc.ignored_pairs = i(ign)
    desc.contact_threshold = float(contact_threshold)
    desc.range = float(range_)
    desc.resolution = float(resolution)
    desc.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    desc.device = int(device)
    return desc, keep, npair_pruned, npair_tightened


def k1_export(*args, **kw) -> dict:
    """Host-only export of what k_is_valid_v5 reads from a scene (mopa_scene_k1_export: no device needed); the arguments are
    those of Scene.  Returns the two blobs, the FP32 pair table, the header bytes, the fingerprint and the launch facts.
    glue=(body_a, body_b) ids: the glued compile (mopa_scene_k1_export_glued; its refusals raise MopaError)."""
    L = lib()
    desc, keep, npruned, ntight = scene_desc(*args, **kw)
    glue = kw.get("glue")
    sizes = np.zeros(8, dtype=np.int64)
    if glue is not None:
        def export(*bufs):
            return L.mopa_scene_k1_export_glued(C.byref(desc), int(glue[0]), int(glue[1]), sizes.ctypes.data_as(C.c_void_p), *bufs)
    else:
        def export(*bufs):
            return L.mopa_scene_k1_export(C.byref(desc), sizes.ctypes.data_as(C.c_void_p), *bufs)
    check(export(None, None, None, None, None))
    dbl = np.zeros(int(sizes[0]), dtype=np.float64)
    ints = np.zeros(int(sizes[1]), dtype=np.int32)
    tab = np.zeros(int(sizes[2]), dtype=np.int32)
    hdr = np.zeros(int(sizes[3]), dtype=np.uint8)
    fp = C.c_uint64()
    check(export(dbl.ctypes.data_as(C.c_void_p), ints.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), hdr.ctypes.data_as(C.c_void_p),
                 C.byref(fp)))
    npair = int(desc.model.npair)
    pairs = np.ctypeslib.as_array(desc.model.pair_geom, shape=(max(npair, 1), 2))[:npair].copy()
    radius = (np.ctypeslib.as_array(desc.pair_cull_radius, shape=(max(npair, 1),))[:npair].copy() if desc.pair_cull_radius
              else np.zeros(npair))
    del keep
    return {"dbl": dbl, "ints": ints, "tab": tab, "hdr": hdr, "fingerprint": int(fp.value), "use_v5": bool(sizes[4]),
            "cen_lds": bool(sizes[5]), "n_mesh_pairs": int(sizes[6]), "nmg": int(sizes[7]),
            "pair_geom": pairs, "pair_cull_radius": radius, "npair_pruned": npruned, "npair_tightened": ntight}


class Scene:
    """Owns one MopaScene* (== one KinematicPlanner instance of the reference)."""

    def __init__(self, model, passive_joint_idx, ignored_contacts, contact_threshold: float, range_: float = 0.1,
                 resolution: float = 0.005, seed: int = 0, device: int = -1, prune_pairs: Optional[bool] = None, glue=None):
        """prune_pairs (default: on, MOPA_PRUNE_PAIRS=0 turns it off): candidate pairs that the scene's compile-time proof
        (tools/prove_separated_pairs.py, `meta["never_violating_pairs"]`: a Lipschitz branch-and-bound over the joint ranges)
        shows can never reach the contact threshold are not handed to the kernels at all.  Verdicts and depths are
        unchanged for joint values inside their ranges inflated by the proof's guard band (`meta["prune_guard_band"]`: 0.05 rad /
        2 mm) -- the states OMPL samples and the rollouts clip to, and what MuJoCo's soft joint limits let through.  The reference's
        isValidState takes ANY state (motion_planners/KinematicPlanner.cpp:253-286): `is_valid_state` here, and `BatchPlanner.
        is_valid(guard=True)`, send a state with a joint beyond range + band through a sibling scene with the full pair list.
        glue = (body_a, body_b), names or ids: the glued scene (mopa_scene_create_glued, include/mopa_hip.h) -- what `glued()` creates."""
        L = lib()
        m = model
        self.glue = None if glue is None else glue_ids(m, *glue)
        self._glued = {}
        self._prune_pairs = prune_pairs
        self._ctor = (model, list(passive_joint_idx), list(ignored_contacts), float(contact_threshold), float(range_), float(resolution), int(seed),
                      int(device))
        self._full = None
        self._h = C.c_void_p()
        # the box inside which the pruning is proven: range + guard band of every limited joint (scenes proven without a band: the range)
        band = getattr(m, "meta", {}).get("prune_guard_band") or {}
        lim = np.asarray(m.jnt_limited).astype(bool) & (np.asarray(m.jnt_type) != 0)
        bw = np.where(np.asarray(m.jnt_type) == 2, float(band.get("slide", 0.0)), float(band.get("hinge", 0.0)))
        self.guard_adr = np.asarray(m.jnt_qposadr, dtype=np.int64)[lim]
        self.guard_lo = (np.asarray(m.jnt_range, dtype=np.float64)[:, 0] - bw)[lim]
        self.guard_hi = (np.asarray(m.jnt_range, dtype=np.float64)[:, 1] + bw)[lim]
        desc, keep, self.npair_pruned, self.npair_tightened = scene_desc(model, passive_joint_idx, ignored_contacts, contact_threshold, range_,
                                                                         resolution, seed, device, prune_pairs, glue=self.glue)
        h = C.c_void_p()
        if self.glue is not None:
            check(L.mopa_scene_create_glued(C.byref(desc), self.glue[0], self.glue[1], C.byref(h)))
        else:
            check(L.mopa_scene_create(C.byref(desc), C.byref(h)))
        self._h = h
        self.model = m
        self.nq = m.nq
        self.na = L.mopa_scene_num_active(h)
        ai = np.zeros(self.na, dtype=np.int32)
        check(L.mopa_scene_active_idx(h, ai.ctypes.data_as(_ip)))
        self.active_idx = ai
        self.npair_checked = L.mopa_scene_num_pairs(h)
        self.lds_bytes = L.mopa_scene_lds_bytes(h)
        self.ngeom = len(m.geom_type)
        self.npair = len(m.pair_geom)
        self.seed = int(seed)
        self.contact_threshold = float(contact_threshold)

    def close(self):
        if getattr(self, "_full", None) is not None:
            self._full.close()
            self._full = None
        for g in list(getattr(self, "_glued", {}).values()):
            g.close()
        self._glued = {}
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().mopa_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def glued(self, body_a, body_b) -> "Scene":
        """the sibling scene that plans with body_b -- the manipulated object, a body with one free joint -- attached to body_a, a
        body the active joints move (names or ids; PyKinematicPlanner's `glue_bodies`).  Created once per pair, closed with this scene.
        It serves is_valid_state / plan here and is_valid / check_motion / plan of BatchPlanner; everything else raises."""
        if self.glue is not None:
            raise MopaError("glued() of a glued scene")
        key = glue_ids(self.model, body_a, body_b)
        if key not in self._glued:
            mdl, pas, ign, thr, rng, res, seed, dev = self._ctor
            self._glued[key] = Scene(mdl, pas, ign, thr, range_=rng, resolution=res, seed=seed, device=dev, prune_pairs=self._prune_pairs, glue=key)
        return self._glued[key]

    @property
    def device_ordinal(self) -> int:
        """the device ordinal this scene was created with; -1: the device that was current at creation"""
        return self._ctor[7]

    def full(self) -> "Scene":
        """the sibling scene with the FULL candidate-pair list (created on first use): where states outside the pruning proof's
        box -- a joint beyond its range + guard band -- are evaluated"""
        if not self.npair_pruned:
            return self
        if self._full is None:
            mdl, pas, ign, thr, rng, res, seed, dev = self._ctor
            self._full = Scene(mdl, pas, ign, thr, range_=rng, resolution=res, seed=seed, device=dev, prune_pairs=False, glue=self.glue)
        return self._full

    def contact_scene(self) -> "Scene":
        """the scene the contact reports run on: this one when it holds the model's whole pair list with no tightened cull
        radius, else the sibling created without pruning (pair indices are then indices into `model.pair_geom`)"""
        if not (self.npair_pruned or self.npair_tightened):
            return self
        if self._full is None:
            mdl, pas, ign, thr, rng, res, seed, dev = self._ctor
            self._full = Scene(mdl, pas, ign, thr, range_=rng, resolution=res, seed=seed, device=dev, prune_pairs=False, glue=self.glue)
        return self._full

    def outside_guard(self, qpos_rows) -> np.ndarray:
        """bool per qpos row: some limited joint lies beyond its range + guard band (the pruned pair list is not proven there)"""
        q = np.atleast_2d(np.asarray(qpos_rows, dtype=np.float64))[:, self.guard_adr]
        return ((q < self.guard_lo) | (q > self.guard_hi)).any(axis=1)

    # ---- single-state forms (host pointers) ----
    def _state(self, qpos):
        """(array, pointer) of one full qpos, shape (nq,)"""
        q, qp = _d(qpos)
        if q.shape != (self.nq,):
            raise MopaError(f"state has dimension {q.shape}, expected nq={self.nq}")
        return q, qp

    @staticmethod
    def _record_bufs(K: int):
        """(count, pair [max(K, 1)] int32, dist [max(K, 1)]) a report row is written into, preset to the unused patterns"""
        return C.c_int32(0), np.full(max(K, 1), -1, dtype=np.int32), np.full(max(K, 1), MOPA_FAR)

    def is_valid_state(self, qpos, want_min_dist: bool = False):
        q, qp = self._state(qpos)
        if self.npair_pruned and bool(self.outside_guard(q)[0]):
            return self.full().is_valid_state(q, want_min_dist)
        v = C.c_int32(0)
        md = C.c_double(0.0)
        check(lib().mopa_is_valid_state(self._h, qp, C.byref(v), C.byref(md) if want_min_dist else None))
        return (bool(v.value), md.value) if want_min_dist else bool(v.value)

    def plan(self, start, goal, max_iters: int, max_nodes: int = 4096, max_path: int = 512, seed: Optional[int] = None,
             env_id: int = 0):
        s, sp = _d(start)
        g, gp = _d(goal)
        prm = MopaPlanParams(int(max_iters), int(max_nodes), int(max_path),
                             int(self.seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF, int(env_id))
        path = np.zeros((max_path, self.nq))
        plen, st, chk = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        check(lib().mopa_plan(self._h, sp, gp, C.byref(prm), path.ctypes.data_as(_dp), C.byref(plen), C.byref(st),
                              C.byref(chk)))
        return st.value, path[:plen.value].copy(), chk.value

    def plan_star(self, start, goal, max_iters: int, max_nodes: Optional[int] = None, max_path: int = 512, seed: Optional[int] = None,
                  env_id: int = 0, goal_bias: float = STAR_GOAL_BIAS, goal_threshold: float = 0.0, rewire_factor: float = STAR_REWIRE_FACTOR):
        """one RRT* query (K3b): -> (status, path rows, cost, info [8] int64); max_nodes=None: max_iters + 1"""
        s, sp = _d(start)
        g, gp = _d(goal)
        nodes = int(max_iters) + 1 if max_nodes is None else int(max_nodes)
        prm = MopaStarParams(int(max_iters), max(nodes, 2), int(max_path), int(self.seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF,
                             int(env_id), None, None, float(goal_bias), float(goal_threshold), float(rewire_factor), 0)
        path = np.zeros((max_path, self.nq))
        info = np.zeros(STAR_INFO_COLS, dtype=np.int64)
        plen, st, cost = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        check(lib().mopa_plan_star(self._h, sp, gp, C.byref(prm), path.ctypes.data_as(_dp), C.byref(plen), C.byref(st), C.byref(cost),
                                   info.ctypes.data_as(C.POINTER(C.c_int64))))
        return st.value, path[:plen.value].copy(), cost.value, info

    def plan_star_clearance(self, start, goal, band: float, max_iters: int, max_nodes: Optional[int] = None, max_path: int = 512,
                            seed: Optional[int] = None, env_id: int = 0, goal_bias: float = STAR_GOAL_BIAS, goal_threshold: float = 0.0,
                            rewire_factor: float = STAR_REWIRE_FACTOR):
        """one RRT* query under the maximize-min-clearance objective at `band` (DESIGN.md "K3b under the clearance objective"):
        -> (status, path rows, clearance, length, info [11] int64); clearance = -inf and length = +inf unless status is 0.
        The planner stays on the inflated (margin-rule) distances: the exact clearance of the returned path is never lower than
        `clearance`, up to kGjkTol = 1e-6; equality of bits with the clearance report holds with exact=False only."""
        s, sp = _d(start)
        g, gp = _d(goal)
        nodes = int(max_iters) + 1 if max_nodes is None else int(max_nodes)
        prm = MopaStarParams(int(max_iters), max(nodes, 2), int(max_path), int(self.seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF,
                             int(env_id), None, None, float(goal_bias), float(goal_threshold), float(rewire_factor), 0)
        path = np.zeros((max_path, self.nq))
        info = np.zeros(STAR_CLEARANCE_INFO_COLS, dtype=np.int64)
        plen, st, clr, length = C.c_int32(0), C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        sc = self if self.glue is not None else self.contact_scene()        # the full pair list, as the clearance report; glue: refused
        check(lib().mopa_plan_star_clearance(sc._h, sp, gp, C.byref(prm), float(band), path.ctypes.data_as(_dp), C.byref(plen), C.byref(st),
                                             C.byref(clr), C.byref(length), info.ctypes.data_as(C.POINTER(C.c_int64))))
        return st.value, path[:plen.value].copy(), clr.value, length.value, info

    def plan_race(self, start, goal, portfolio: int, max_iters: int, max_nodes: int = 4096, max_path: int = 512, seed: Optional[int] = None,
                  env_id: int = 0, no_abort: bool = False):
        """one RRT-Connect query run by `portfolio` members that differ in their seed only (K3 race): -> (status, path rows,
        the winner's consumed checks, winner, the winner's seed, info [3] int64 = members cut, checks spent by all members, the
        winner's iterations); without a solved member winner = -1 and checks / seed are member 0's"""
        s, sp = _d(start)
        g, gp = _d(goal)
        prm = MopaRaceParams(int(max_iters), int(max_nodes), int(max_path), int(portfolio), int(self.seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF,
                             int(env_id), None, None, 0, 1 if no_abort else 0)
        path = np.zeros((max_path, self.nq))
        info = np.zeros(RACE_INFO_COLS, dtype=np.int64)
        plen, st, chk, win, wseed = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int32(0), C.c_uint64(0)
        check(lib().mopa_plan_race(self._h, sp, gp, C.byref(prm), path.ctypes.data_as(_dp), C.byref(plen), C.byref(st), C.byref(chk), C.byref(win),
                                   C.byref(wseed), info.ctypes.data_as(C.POINTER(C.c_int64))))
        return st.value, path[:plen.value].copy(), chk.value, win.value, wseed.value, info

    def valid_kernel(self, n_states: int) -> str:
        """name of the validity kernel `mopa_is_valid_batch` dispatches for a batch of n_states"""
        buf = C.create_string_buffer(32)
        check(lib().mopa_scene_valid_kernel(self._h, int(n_states), buf, 32))
        return buf.value.decode()

    def motion_kernel(self, n_segments: int) -> str:
        """the form `mopa_check_motion_batch` takes for n_segments: "k_check_motion" or "k_motion_expand" """
        buf = C.create_string_buffer(32)
        check(lib().mopa_scene_motion_kernel(self._h, int(n_segments), buf, 32))
        return buf.value.decode()

    def planner_status(self) -> bytes:
        return lib().mopa_planner_status(self._h)

    def debug_fk(self, qpos):
        q, qp = _d(qpos)
        gpos = np.zeros((self.ngeom, 3)); gmat = np.zeros((self.ngeom, 9))
        check(lib().mopa_debug_fk(self._h, qp, gpos.ctypes.data_as(_dp), gmat.ctypes.data_as(_dp)))
        return gpos, gmat.reshape(-1, 3, 3)

    def contacts_state_raw(self, qpos, cutoff: Optional[float] = None, max_contacts: int = 64):
        """(count, pair [K] int32, dist [K]) of one state: the single-state form of `BatchPlanner.contacts`"""
        sc = self.contact_scene()
        q, qp = self._state(qpos)
        K = int(max_contacts)
        cnt, pair, dist = self._record_bufs(K)
        check(lib().mopa_contacts_state(sc._h, qp, float(self.contact_threshold if cutoff is None else cutoff), K, C.byref(cnt),
                                        pair.ctypes.data_as(_ip), dist.ctypes.data_as(_dp)))
        return int(cnt.value), pair, dist

    def contact_frames_state_raw(self, qpos, cutoff: Optional[float] = None, max_contacts: int = 64):
        """(count, pair [K] int32, dist [K], normal [K, 3], pos [K, 3]) of one state: `contacts_state_raw` with the contact
        frame of every record (mopa_contact_frames_state); unused slots of normal / pos hold 0.0"""
        sc = self.contact_scene()
        q, qp = self._state(qpos)
        K = int(max_contacts)
        cnt, pair, dist = self._record_bufs(K)
        normal = np.zeros((max(K, 1), 3))
        pos = np.zeros((max(K, 1), 3))
        check(lib().mopa_contact_frames_state(sc._h, qp, float(self.contact_threshold if cutoff is None else cutoff), K, C.byref(cnt),
                                              pair.ctypes.data_as(_ip), dist.ctypes.data_as(_dp), normal.ctypes.data_as(_dp), pos.ctypes.data_as(_dp)))
        return int(cnt.value), pair, dist, normal, pos

    def contact_manifolds_state_raw(self, qpos, cutoff: Optional[float] = None, max_contacts: int = 64, max_points: int = 4, point_cutoff: float = 0.0):
        """(count, pair [K] int32, dist [K], normal [K, 3], npoint [K] int32, point_dist [K, P], point_pos [K, P, 3]) of one
        state: `contacts_state_raw` with the contact manifold of every record (mopa_contact_manifolds_state); unused slots hold
        normal / npoint / point_pos 0, point_dist MOPA_FAR"""
        sc = self.contact_scene()
        q, qp = self._state(qpos)
        K, P = int(max_contacts), int(max_points)
        k1, p1 = max(K, 1), max(P, 1)
        cnt, pair, dist = self._record_bufs(K)
        normal = np.zeros((k1, 3))
        npoint = np.zeros(k1, dtype=np.int32)
        pdist = np.full((k1, p1), MOPA_FAR)
        ppos = np.zeros((k1, p1, 3))
        check(lib().mopa_contact_manifolds_state(sc._h, qp, float(self.contact_threshold if cutoff is None else cutoff), float(point_cutoff), K, P,
                                                 C.byref(cnt), pair.ctypes.data_as(_ip), dist.ctypes.data_as(_dp), normal.ctypes.data_as(_dp),
                                                 npoint.ctypes.data_as(_ip), pdist.ctypes.data_as(_dp), ppos.ctypes.data_as(_dp)))
        return int(cnt.value), pair, dist, normal, npoint, pdist, ppos

    def contacts_state(self, qpos, cutoff: Optional[float] = None, frames: bool = False, manifold: bool = False, max_points: int = 4,
                       point_cutoff: float = 0.0):
        """The pairs in contact in one state, as the reference's checker sees them in `d->contact[i]`: a list of
        (geom1_name, geom2_name, dist) over the non-ignored candidate pairs with dist <= cutoff, in `model.pair_geom` order.
        cutoff=None: the scene's contact_threshold -- the pairs that make the state invalid.  cutoff must be < 0.
        frames=True: (geom1_name, geom2_name, dist, normal, pos) -- ONE contact frame per pair, that of the deepest contact
        (MuJoCo may emit several contacts for a pair): `normal` [3] a unit vector from geom1 towards geom2, `pos` [3] the
        midpoint of the two witness points ("Contact frames").
        manifold=True (takes precedence over frames): (geom1_name, geom2_name, dist, normal, [(pos, dist_i), ...]) -- the same
        normal and up to max_points (1..8) contact points with dist_i <= point_cutoff, deepest first (DESIGN.md section 4,
        "Contact manifolds"; PARITY UNPINNED)."""
        m = self.model
        K = max(1, len(m.pair_geom))
        if manifold:
            n, pair, dist, normal, npoint, pdist, ppos = self.contact_manifolds_state_raw(qpos, cutoff, K, max_points, point_cutoff)
            return [rec + (normal[k].copy(), [(ppos[k, j].copy(), float(pdist[k, j])) for j in range(min(int(npoint[k]), pdist.shape[1]))])
                    for k, rec in enumerate(_pair_names(m, pair, dist, n))]
        if frames:
            n, pair, dist, normal, pos = self.contact_frames_state_raw(qpos, cutoff, K)
            return [rec + (normal[k].copy(), pos[k].copy()) for k, rec in enumerate(_pair_names(m, pair, dist, n))]
        n, pair, dist = self.contacts_state_raw(qpos, cutoff, K)
        return _pair_names(m, pair, dist, n)

    def proximity_state_raw(self, qpos, band: float, max_pairs: int = 8, exact: bool = False, witness: bool = False):
        """(clearance, count, pair [K] int32, dist [K]) of one state: the single-state form of `BatchPlanner.proximity`
        (exact=True: mopa_proximity_exact_state).  witness=True (needs exact=True; mopa_proximity_witness_state): three more
        entries normal, p1, p2 [K, 3], 0.0 in unused slots"""
        if witness and not exact:
            raise ValueError("witness=True needs exact=True: the inflated route's distance is not attained by two points of the shapes")
        if self.glue is not None:
            raise NotImplementedError("the proximity report of a glued scene")
        sc = self.contact_scene()
        q, qp = self._state(qpos)
        K = int(max_pairs)
        cl = C.c_double(0.0)
        cnt, pair, dist = self._record_bufs(K)
        if witness:
            normal, p1, p2 = (np.zeros((max(K, 1), 3)) for _ in range(3))
            check(lib().mopa_proximity_witness_state(sc._h, qp, float(band), K, C.byref(cl), C.byref(cnt), pair.ctypes.data_as(_ip), dist.ctypes.data_as(_dp),
                                                     normal.ctypes.data_as(_dp), p1.ctypes.data_as(_dp), p2.ctypes.data_as(_dp)))
            return float(cl.value), int(cnt.value), pair, dist, normal, p1, p2
        fn = lib().mopa_proximity_exact_state if exact else lib().mopa_proximity_state
        check(fn(sc._h, qp, float(band), K, C.byref(cl), C.byref(cnt), pair.ctypes.data_as(_ip), dist.ctypes.data_as(_dp)))
        return float(cl.value), int(cnt.value), pair, dist

    def proximity_state(self, qpos, band: float, max_pairs: int = 8, exact: bool = False, witness: bool = False):
        """How far from collision one state is, and which pairs are nearest: -> (clearance, [(geom1_name, geom2_name, dist), ...]),
        clearance = min(band, the smallest pair distance), the list the at most max_pairs nearest non-ignored candidate pairs with
        dist <= band, nearest first.  Distances of disjoint box-box, cylinder and mesh pairs are conservative -- never more than 1e-6
        above the true distance, below it by a shortfall that grows with band ("Proximity report").
        exact=True: those pairs get their GJK distance instead, true <= d <= true + 1e-6 whatever the band ("Exact route").
        witness=True (needs exact=True): (geom1_name, geom2_name, dist, normal, p1, p2) -- `p1` [3] a point of geom1 and `p2` [3] a
        point of geom2 at that distance from each other, `normal` [3] the unit vector from p1 towards p2; for a pair in overlap the
        contact frame's normal and its two witness points ("Witness points")."""
        if witness:
            cl, n, pair, dist, normal, p1, p2 = self.proximity_state_raw(qpos, band, max_pairs, exact, True)
            return cl, [rec + (normal[k].copy(), p1[k].copy(), p2[k].copy()) for k, rec in enumerate(_pair_names(self.model, pair, dist, n))]
        cl, n, pair, dist = self.proximity_state_raw(qpos, band, max_pairs, exact)
        return cl, _pair_names(self.model, pair, dist, n)

    def motion_report_raw(self, qpos_a, qpos_b, max_contacts: int = 0):
        """(valid, n_states, first_bad, last_valid_t, last_valid_q [na], first_bad_q [na], blockers) of one segment: the
        single-segment form of `BatchPlanner.motion_report` (mopa_motion_report) from the active entries of qpos_a to those of
        qpos_b, the passive entries taken from qpos_a.  blockers: None with max_contacts = 0, else (count, pair [K] int32,
        dist [K]) of the state first_bad_q at the contact threshold, pair indices into `model.pair_geom` -- in the same call on a
        scene that holds the whole pair list, else through the sibling `contact_scene()` (the same bytes)."""
        (a, ap), (b, bp) = self._state(qpos_a), self._state(qpos_b)
        K = int(max_contacts)
        chained = K != 0 and self.contact_scene() is self
        v, n, fb, t = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        lvq, fbq = np.zeros(self.na), np.zeros(self.na)
        cnt, pair, dist = self._record_bufs(K)
        if K < 0:
            raise MopaError("max_contacts must be >= 0")
        check(lib().mopa_motion_report(self._h, ap, bp, C.byref(v), C.byref(n), C.byref(fb), C.byref(t), lvq.ctypes.data_as(_dp), fbq.ctypes.data_as(_dp),
                                       K if chained else 0, C.byref(cnt) if chained else None, pair.ctypes.data_as(_ip) if chained else None,
                                       dist.ctypes.data_as(_dp) if chained else None))
        blockers = None
        if chained:
            blockers = (int(cnt.value), pair, dist)
        elif K:
            q = a.copy()
            q[self.active_idx] = fbq
            blockers = self.contacts_state_raw(q, None, K)
        return bool(v.value), int(n.value), int(fb.value), float(t.value), lvq, fbq, blockers

    def motion_report_state(self, qpos_a, qpos_b, max_contacts: int = 0):
        """Where the straight line from qpos_a to qpos_b is blocked, and by what: OMPL's checkMotion(s1, s2, lastValid) over the
        states s_k, k = 1 .. n_states (s_k at k / n_states along the segment, the last one qpos_b's active entries; qpos_a is
        not tested).  -> dict: `valid`, `n_states`, `first_bad` (the smallest k with s_k invalid, 0 if valid), `last_valid_t`
        ((first_bad - 1) / n_states, 1.0 if valid), `last_valid_q` / `first_bad_q` (active coordinates [na]; both qpos_b's if valid)
        and `blockers`: None with max_contacts = 0, else the pairs that make s_first_bad invalid as (geom1_name, geom2_name,
        dist), at most max_contacts of them in `model.pair_geom` order (the style of `contacts_state`), and `n_blockers`, their
        uncapped number.  DESIGN.md section 4, "Motion report"."""
        valid, n, fb, t, lvq, fbq, blk = self.motion_report_raw(qpos_a, qpos_b, max_contacts)
        out = {"valid": valid, "n_states": n, "first_bad": fb, "last_valid_t": t, "last_valid_q": lvq, "first_bad_q": fbq, "blockers": None}
        if blk is not None:
            cnt, pair, dist = blk
            out["blockers"] = _pair_names(self.model, pair, dist, cnt)
            out["n_blockers"] = cnt
        return out

    def motion_clearance_raw(self, qpos_a, qpos_b, band: float, exact: bool = False):
        """(clearance, n_states, n_near, k_min, t_min, pair_min, end_clearance, q_min [na]) of one segment: the single-segment
        form of `BatchPlanner.motion_clearance` (mopa_motion_clearance) from the active entries of qpos_a to those of qpos_b, the
        passive entries taken from qpos_a; pair_min is an index into `model.pair_geom` (-1: nothing within the band).
        exact=True: mopa_motion_clearance_exact, the per-state distances of `proximity(exact=True)`."""
        if self.glue is not None:
            raise NotImplementedError("the clearance report of a glued scene")
        sc = self.contact_scene()
        (a, ap), (b, bp) = self._state(qpos_a), self._state(qpos_b)
        cl, t, ec = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        n, near, k, pair = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        q_min = np.zeros(self.na)
        fn = lib().mopa_motion_clearance_exact if exact else lib().mopa_motion_clearance
        check(fn(sc._h, ap, bp, float(band), C.byref(cl), C.byref(n), C.byref(near), C.byref(k), C.byref(t), C.byref(pair), C.byref(ec),
                 q_min.ctypes.data_as(_dp)))
        return float(cl.value), int(n.value), int(near.value), int(k.value), float(t.value), int(pair.value), float(ec.value), q_min

    def motion_clearance_state(self, qpos_a, qpos_b, band: float, exact: bool = False):
        """How near the straight line from qpos_a to qpos_b comes to collision, where, and to which pair: OMPL's
        MinimaxObjective::motionCost under the clearance state cost, over the states s_k, k = 1 .. n_states, `motion_report_state`
        walks (qpos_a is not evaluated).  -> dict: `clearance` (the smallest state clearance, saturating at band), `n_states`,
        `n_near` (states with a pair within the band), `k_min` (the first state that attains the clearance, 0: nothing within the
        band), `t_min` (k_min / n_states), `pair` ((geom1_name, geom2_name) of the nearest pair there, None when k_min == 0),
        `pair_min` (its index into `model.pair_geom`, -1), `end_clearance` (that of qpos_b) and `q_min` (active coordinates [na] of
        s_k_min; qpos_b's when k_min == 0).  exact=True: the state clearances of `proximity_state(exact=True)`.  DESIGN.md section 4,
        "Clearance report"."""
        cl, n, near, k, t, pair, ec, q_min = self.motion_clearance_raw(qpos_a, qpos_b, band, exact)
        return {"clearance": cl, "n_states": n, "n_near": near, "k_min": k, "t_min": t, "pair_min": pair,
                "pair": _pair_names(self.model, [pair], [cl], 1)[0][:2] if pair >= 0 else None, "end_clearance": ec, "q_min": q_min}

    def debug_pair_dist(self, qpos):
        q, qp = _d(qpos)
        out = np.zeros(self.npair)
        check(lib().mopa_debug_pair_dist(self._h, qp, out.ctypes.data_as(_dp)))
        return out
