"""ctypes binding of libmind_hip.so (C-ABI in include/mind_hip.h).

The product path has NO CPU fallback: if the HIP library is missing this raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIND_HIP_LIB", os.path.join(_HERE, "libmind_hip.so"))   # override: diagnostic builds only

WAIT_CLOCK = C.CFUNCTYPE(C.c_double, C.c_void_p)      # mind_debug_wait_word's clock
MIND_OK = 0
MIND_EINVAL, MIND_ENOMEM, MIND_EHIP, MIND_ESTATE, MIND_ENOTFOUND = -1, -2, -3, -4, -5     # include/mind_hip.h:21-25


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class SceneBatch(C.Structure):
    _fields_ = [("n_scenes", C.c_int), ("actor_off", C.POINTER(C.c_int32)), ("lane_off", C.POINTER(C.c_int32)),
                ("actors", C.c_void_p), ("lanes", C.c_void_p), ("lane_feat", C.c_void_p),
                ("actor_ctrs", C.c_void_p), ("actor_vecs", C.c_void_p), ("lane_ctrs", C.c_void_p),
                ("lane_vecs", C.c_void_p), ("rpe", C.POINTER(C.c_void_p)), ("tgt_nodes", C.c_void_p),
                ("tgt_rpe", C.c_void_p)]


class PredOut(C.Structure):
    _fields_ = [("cls", C.c_void_p), ("reg", C.c_void_p), ("vel", C.c_void_p), ("lane_feat", C.c_void_p),
                ("actor_emb", C.c_void_p), ("cls_emb", C.c_void_p)]


class PredAux(C.Structure):         # mind_pred_aux
    _fields_ = [("cov_vel", C.c_void_p), ("param", C.c_void_p)]


BASIS = ("bezier", "monomial")      # MIND_BASIS_*: SceneDecoder's param_out


class CostTree(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("parent", C.POINTER(C.c_int32)), ("prob", C.POINTER(C.c_float)),
                ("n_agents", C.c_int), ("agent_mean", C.POINTER(C.c_float)), ("agent_cov", C.POINTER(C.c_float)),
                ("field", C.POINTER(C.c_double)), ("node_w", C.POINTER(C.c_double))]


class FieldGrid(C.Structure):
    _fields_ = [("W", C.c_int), ("H", C.c_int), ("res", C.c_double), ("off_x", C.c_double), ("off_y", C.c_double),
                ("gx", C.POINTER(C.c_double)), ("gy", C.POINTER(C.c_double))]


class IlqrGainsOut(C.Structure):     # mind_ilqr_gains_out
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("k", "K", "dV", "V_x", "V_xx", "xs", "L", "J")] + [("bad_node", C.POINTER(C.c_int32))]


class AuditBox(C.Structure):        # mind_audit_box
    _fields_ = [("length", C.c_double), ("width", C.c_double), ("center_offset", C.c_double)]


class AuditPlanOut(C.Structure):    # mind_audit_plan_out
    _fields_ = [("node_clear", C.POINTER(C.c_double)), ("node_agent", C.POINTER(C.c_int32)), ("tree_min", C.POINTER(C.c_double)),
                ("tree_node", C.POINTER(C.c_int32)), ("tree_agent", C.POINTER(C.c_int32)), ("tree_hits", C.POINTER(C.c_int32)),
                ("tree_first", C.POINTER(C.c_int32)), ("tree_mass", C.POINTER(C.c_double))]


class AuditEpisodeOut(C.Structure):     # mind_audit_episode_out
    _fields_ = [("step_clear", C.POINTER(C.c_double)), ("step_track", C.POINTER(C.c_int32)), ("ego_min", C.POINTER(C.c_double)),
                ("ego_step", C.POINTER(C.c_int32)), ("ego_track", C.POINTER(C.c_int32)), ("ego_hits", C.POINTER(C.c_int32)),
                ("ego_first", C.POINTER(C.c_int32))]


class AuditRoadPlanOut(C.Structure):    # mind_audit_road_plan_out
    _fields_ = [("node_margin", C.POINTER(C.c_double)), ("node_corner", C.POINTER(C.c_int32)), ("node_ring", C.POINTER(C.c_int32)),
                ("node_edge", C.POINTER(C.c_int32)), ("tree_min", C.POINTER(C.c_double)), ("tree_node", C.POINTER(C.c_int32)),
                ("tree_corner", C.POINTER(C.c_int32)), ("tree_hits", C.POINTER(C.c_int32)), ("tree_first", C.POINTER(C.c_int32)),
                ("tree_mass", C.POINTER(C.c_double))]


class AuditRoadEpisodeOut(C.Structure):     # mind_audit_road_episode_out
    _fields_ = [("step_margin", C.POINTER(C.c_double)), ("step_corner", C.POINTER(C.c_int32)), ("step_ring", C.POINTER(C.c_int32)),
                ("step_edge", C.POINTER(C.c_int32)), ("ego_min", C.POINTER(C.c_double)), ("ego_step", C.POINTER(C.c_int32)),
                ("ego_corner", C.POINTER(C.c_int32)), ("ego_hits", C.POINTER(C.c_int32)), ("ego_first", C.POINTER(C.c_int32))]


class AuditTtcCfg(C.Structure):     # mind_audit_ttc_cfg
    _fields_ = [("horizon", C.c_double), ("bound", C.c_double), ("lanes", C.c_int)]


class AuditTtcOut(C.Structure):     # mind_audit_ttc_out
    _fields_ = [("step_ttc", C.POINTER(C.c_double)), ("step_track", C.POINTER(C.c_int32)), ("ego_min", C.POINTER(C.c_double)),
                ("ego_step", C.POINTER(C.c_int32)), ("ego_track", C.POINTER(C.c_int32)), ("ego_hits", C.POINTER(C.c_int32)),
                ("ego_first", C.POINTER(C.c_int32))]


class AuditLaneCfg(C.Structure):    # mind_audit_lane_cfg
    _fields_ = [("cos_flow", C.c_double), ("bound", C.c_double), ("form", C.c_int)]


def _lane_out(per, outer, extra):
    """the field list of mind_audit_lane_episode_out (per = "step", outer = "ego") / mind_audit_lane_plan_out ("node", "tree")"""
    dbl, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    return [(f"{per}_{k}", dbl) for k in ("lat", "s", "along", "across")] + [(f"{per}_lane", i32), (f"{per}_edge", i32), (f"{per}_margin", dbl)] + \
        [(f"{outer}_min", dbl), (f"{outer}_{per}", i32), (f"{outer}_lane", i32), (f"{outer}_hits", i32), (f"{outer}_first", i32)] + [(k, dbl) for k in extra]


class AuditLaneEpisodeOut(C.Structure):     # mind_audit_lane_episode_out
    _fields_ = _lane_out("step", "ego", ("ego_progress", "ego_back"))


class AuditLanePlanOut(C.Structure):    # mind_audit_lane_plan_out
    _fields_ = _lane_out("node", "tree", ("tree_mass", "tree_progress"))


class ForecastCfg(C.Structure):     # mind_forecast_cfg
    _fields_ = [("K", C.c_int), ("T", C.c_int), ("n_h", C.c_int), ("horizon", C.POINTER(C.c_int32)), ("miss_radius", C.c_double),
                ("disc_scale", C.c_double), ("disc_offset", C.c_double)]


# mind_forecast_out, in its field order: name -> (dtype, "a" = per agent / "s" = per scene, trailing K axis)
FORECAST_OUT = (("ade", "f8", "a", True), ("fde", "f8", "a", True), ("cover", "i4", "a", True), ("first_out", "i4", "a", True),
                ("n_valid", "i4", "a", False), ("last", "i4", "a", False), ("k_ade", "i4", "a", False), ("k_fde", "i4", "a", False),
                ("brier_fde", "f8", "a", False), ("s_n_scored", "i4", "s", False), ("s_ade", "f8", "s", True), ("s_fde", "f8", "s", True),
                ("s_k_ade", "i4", "s", False), ("s_k_fde", "i4", "s", False), ("s_k_top", "i4", "s", False), ("s_brier_fde", "f8", "s", False),
                ("s_miss_rate", "f8", "s", False), ("s_miss_top", "f8", "s", False))


class ForecastOut(C.Structure):     # mind_forecast_out
    _fields_ = [(n, C.POINTER(C.c_double if dt == "f8" else C.c_int32)) for n, dt, _, _ in FORECAST_OUT]


class WorldIn(C.Structure):
    _fields_ = [("n_scenes", C.c_int), ("actor_off", C.POINTER(C.c_int32)), ("reg", C.c_void_p), ("vel", C.c_void_p),
                ("actor_ctrs", C.c_void_p), ("actor_vecs", C.c_void_p), ("rot", C.POINTER(C.c_float)),
                ("orig", C.POINTER(C.c_float)), ("cov_last", C.POINTER(C.c_float)), ("last", C.POINTER(C.c_int32)),
                ("target_lane", C.POINTER(C.c_float)), ("n_lane_pts", C.c_int), ("cls", C.c_void_p),
                ("scen_prob", C.POINTER(C.c_float)), ("lane_check", C.c_int), ("dist_thres", C.c_float)]


class WorldOut(C.Structure):
    _fields_ = [("world", C.c_void_p), ("topo", C.c_void_p), ("ego_end", C.c_void_p), ("sel", C.c_void_p), ("sel_prob", C.c_void_p)]


class RebaseIn(C.Structure):
    _fields_ = [("n_scenes", C.c_int), ("n_agents", C.c_int), ("n_lanes", C.c_int), ("pos", C.POINTER(C.c_float)),
                ("ang", C.POINTER(C.c_float)), ("vel", C.POINTER(C.c_float)), ("types", C.POINTER(C.c_float)),
                ("pad", C.POINTER(C.c_float)), ("lane_ctrs", C.POINTER(C.c_float)), ("lane_vecs", C.POINTER(C.c_float)),
                ("target_lane", C.POINTER(C.c_float)), ("target_lane_info", C.POINTER(C.c_float)), ("n_lane_pts", C.c_int),
                ("time_ahead", C.c_float), ("min_vel", C.c_float), ("rows_dev", C.c_void_p), ("parent_slot", C.POINTER(C.c_int32)),
                ("row0", C.POINTER(C.c_int32)), ("dur", C.POINTER(C.c_int32)), ("prev_gen", C.c_int)]


class RebaseOut(C.Structure):
    _fields_ = [("actors", C.c_void_p), ("actor_ctrs", C.c_void_p), ("actor_vecs", C.c_void_p), ("lane_ctrs", C.c_void_p),
                ("lane_vecs", C.c_void_p), ("tgt_nodes", C.c_void_p), ("tgt_rpe", C.c_void_p), ("frames", C.c_void_p),
                ("gen", C.POINTER(C.c_int32))]


class AimePlanIn(C.Structure):
    _fields_ = [("n_agents", C.c_int), ("n_lanes", C.c_int), ("n_lane_pts", C.c_int)] + \
               [(k, C.POINTER(C.c_float)) for k in ("actors", "actor_ctrs", "actor_vecs", "lanes", "lane_ctrs", "lane_vecs", "tgt_nodes", "tgt_rpe",
                                                    "rot", "orig", "tgt_pts", "hist", "types", "target_lane", "target_lane_info")] + \
               [("time_ahead", C.c_float), ("min_vel", C.c_float), ("dist_thres", C.c_float), ("max_depth", C.c_int), ("max_rounds", C.c_int), ("pred_len", C.c_int),
                ("raw_pos", C.POINTER(C.c_float)), ("raw_ang", C.POINTER(C.c_float)), ("raw_vel", C.POINTER(C.c_float)), ("raw_pad", C.POINTER(C.c_float)),
                ("lane_pts", C.POINTER(C.c_double)), ("lane_flags", C.POINTER(C.c_int32)), ("travel0", C.c_float),
                ("script_cls", C.c_void_p), ("script_reg", C.c_void_p), ("script_vel", C.c_void_p), ("prob_floor", C.c_float),
                ("solve_cfg_warm", C.c_void_p), ("solve_cfg_full", C.c_void_p), ("solve_x0", C.c_void_p), ("solve_lane", C.c_void_p),
                ("solve_n_lane_pts", C.c_int), ("solve_target_vel", C.c_double)]


class AimeNode(C.Structure):
    _fields_ = [("round", C.c_int), ("scene", C.c_int), ("mode", C.c_int), ("parent", C.c_int), ("prob", C.c_float),
                ("cur_t", C.c_int), ("end_t", C.c_int), ("flags", C.c_int), ("dur", C.c_int), ("row_off", C.c_int64),
                ("tgt_pts", C.c_float * 22)]


class AimePlanOut(C.Structure):
    _fields_ = [("nodes", C.POINTER(AimeNode)), ("n_nodes", C.c_int), ("rows", C.POINTER(C.c_float)), ("n_row_floats", C.c_int64),
                ("n_expanded", C.c_int), ("n_rounds", C.c_int), ("root_flags", C.c_int), ("round_scenes", C.c_int * 32),
                ("pair_ms", C.c_float), ("pair_launches", C.c_int), ("n_trees", C.c_int), ("tree_top", C.POINTER(C.c_int32)),
                ("tree_off", C.POINTER(C.c_int32)), ("flat_parent", C.POINTER(C.c_int32)), ("flat_prob", C.POINTER(C.c_float)),
                ("flat_mean", C.POINTER(C.c_float)), ("flat_cov", C.POINTER(C.c_float)), ("solves_begun", C.c_int)]


class IlqrCfg(C.Structure):
    _fields_ = [("dt", C.c_double), ("wheelbase", C.c_double), ("w_des_state", C.c_double * 6),
                ("w_state_con", C.c_double * 6), ("state_lower", C.c_double * 6), ("state_upper", C.c_double * 6),
                ("w_ctrl", C.c_double * 2), ("w_tgt", C.c_double), ("w_ego", C.c_double),
                ("w_ego_cov_offset", C.c_double), ("w_exo", C.c_double), ("w_exo_cov_offset", C.c_double),
                ("w_exo_cost_offset", C.c_double), ("grid_res", C.c_double), ("grid_w", C.c_int), ("grid_h", C.c_int),
                ("max_iter", C.c_int)]


class IlqrStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("J", C.c_double), ("mu", C.c_double)]


LOOP_TAN_FN = C.CFUNCTYPE(C.c_double, C.c_double)                       # mind_loop_desc.tan_fn / .sincos_fn
LOOP_SINCOS_FN = C.CFUNCTYPE(None, C.c_double, C.POINTER(C.c_double))


class LoopDesc(C.Structure):       # mind_loop_desc (include/mind_hip.h)
    _fields_ = [("n_tracks", C.c_int), ("n_steps", C.c_int), ("clamp_last", C.c_int), ("ego_state", C.c_void_p), ("ego_state_is_f32", C.c_int), ("ego_obs", C.c_void_p), ("ego_trig32", C.c_void_p),
                ("tan_fn", C.c_void_p), ("sincos_fn", C.c_void_p), ("exo_obs", C.c_void_p),
                ("exo_valid", C.c_void_p), ("timestep", C.c_void_p), ("type_slot", C.c_void_p),
                ("sim_step", C.c_double), ("plan_step", C.c_double), ("enable_time", C.c_double),
                ("wheelbase", C.c_double), ("max_speed", C.c_double), ("max_steer", C.c_double), ("max_acc", C.c_double), ("max_dec", C.c_double),
                ("n_lanes", C.c_int), ("lane_pts", C.c_void_p), ("lane_flags", C.c_void_p),
                ("n_lane_pts", C.c_int), ("target_lane", C.c_void_p), ("target_lane_info", C.c_void_p),
                ("time_ahead", C.c_double), ("min_vel", C.c_float), ("dist_thres", C.c_float), ("max_depth", C.c_int), ("max_rounds", C.c_int),
                ("pred_len", C.c_int), ("prob_floor", C.c_float),
                ("cfg_warm", C.c_void_p), ("cfg_full", C.c_void_p), ("solve_n_lane_pts", C.c_int), ("solve_lane", C.c_void_p), ("target_vel", C.c_double),
                ("eval_n_lane_pts", C.c_int), ("eval_lane_is_f32", C.c_int), ("eval_lane", C.c_void_p), ("speculative", C.c_int)]


class LoopTotals(C.Structure):     # mind_loop_totals
    _fields_ = [("plans", C.c_longlong), ("expansions", C.c_longlong), ("scen_trees", C.c_longlong), ("rounds", C.c_longlong),
                ("aime_s", C.c_double), ("ilqr_s", C.c_double), ("total_s", C.c_double),
                ("iterations", C.c_longlong), ("node_iterations", C.c_longlong), ("node_iterations_exo", C.c_longlong),
                ("warm_speculated", C.c_longlong), ("warm_hits", C.c_longlong),
                ("pair_ms", C.c_double), ("pair_launches", C.c_longlong), ("scene_n2", C.c_double), ("scene_n_a1", C.c_double),
                ("ilqr_ms", C.c_double), ("ilqr_launches", C.c_longlong), ("ilqr_trees", C.c_longlong), ("ilqr_workgroups_per_tree", C.c_int),
                ("ilqr_prof", C.c_double * 9), ("ilqr_node_steps", C.c_double)]


class LoopOut(C.Structure):        # mind_loop_out
    _fields_ = [("planned", C.c_int), ("enabled", C.c_int), ("n_steps", C.c_longlong), ("n_plans", C.c_longlong), ("episode_steps", C.c_longlong),
                ("sim_time", C.c_double), ("last_trigger", C.c_double), ("state", C.c_double * 4), ("ctrl", C.c_double * 2),
                ("n_agents", C.c_int), ("n_trees", C.c_int), ("best", C.c_int), ("n_expanded", C.c_int), ("n_rounds", C.c_int), ("n_traj_nodes", C.c_int),
                ("costs", C.POINTER(C.c_double)), ("aime_s", C.c_double), ("ilqr_s", C.c_double), ("total_s", C.c_double),
                ("tot", LoopTotals)]


PLANNER_EGO_KEY = -(1 << 63)        # MIND_PLANNER_EGO_KEY


class PlannerDesc(C.Structure):    # mind_planner_desc
    _fields_ = [("time_ahead", C.c_double), ("min_vel", C.c_float), ("dist_thres", C.c_float), ("max_depth", C.c_int), ("max_rounds", C.c_int),
                ("pred_len", C.c_int), ("prob_floor", C.c_float), ("cfg_warm", C.c_void_p), ("cfg_full", C.c_void_p), ("speculative", C.c_int),
                ("ego_type_slot", C.c_int)]


class PlannerOut(C.Structure):     # mind_planner_out
    _fields_ = [("n_plans", C.c_longlong),
                ("n_agents", C.c_int), ("n_trees", C.c_int), ("best", C.c_int), ("n_expanded", C.c_int), ("n_rounds", C.c_int), ("n_traj_nodes", C.c_int),
                ("costs", C.POINTER(C.c_double)), ("ctrl", C.c_double * 2), ("aime_s", C.c_double), ("ilqr_s", C.c_double), ("total_s", C.c_double),
                ("tot", LoopTotals)]


EXPORTS = ["mind_ctx_create", "mind_ctx_destroy", "mind_last_error_string", "mind_ctx_synchronize",
           "mind_weights_load", "mind_predict_batch", "mind_last_fusion_stats", "mind_last_actor_stats", "mind_debug_actor_lw_plan", "mind_last_token_stats", "mind_last_token_stage_ms", "mind_debug_token_lw_plan", "mind_set_profiling", "mind_debug_launch_times", "mind_debug_launch_clock",
           "mind_ilqr_solve_trees", "mind_ilqr_contingency", "mind_ilqr_solve_fields", "mind_cost_eval", "mind_ilqr_score_trees", "mind_ilqr_gains", "mind_ilqr_policy_rollouts", "mind_lane_dist_field", "mind_aime_world", "mind_aime_rebase", "mind_debug_aime_decide", "mind_debug_set_layers", "mind_debug_token_form",
           "mind_debug_read", "mind_set_pair_precision", "mind_get_pair_precision", "mind_debug_pack_bfrag", "mind_debug_pack_conv_frag", "mind_debug_pack", "mind_debug_weight_image", "mind_debug_weight_bind", "mind_debug_pair_schedule", "mind_debug_predict_choice", "mind_debug_ilqr_plan", "mind_debug_aime_book", "mind_set_tuning", "mind_get_tuning", "mind_debug_tuning", "mind_debug_live_handles", "mind_last_ilqr_stats", "mind_aime_plan", "mind_last_ilqr_profile", "mind_eval_traj_trees", "mind_last_ilqr_trace", "mind_ilqr_contingency_begin", "mind_ilqr_finish", "mind_fill_tracks", "mind_ilqr_contingency_begin_plan", "mind_debug_trig", "mind_aime_plan_begin", "mind_aime_plan_poll", "mind_aime_plan_finish", "mind_ctx_busy", "mind_ilqr_finish_plan", "mind_debug_dec_scene",
           "mind_set_exchange", "mind_last_exchange_stats", "mind_debug_wait_word",
           "mind_predict_batch_aux", "mind_set_decoder_basis", "mind_get_decoder_basis", "mind_curve_eval", "mind_debug_curve_basis",
           "mind_audit_plan", "mind_audit_episode", "mind_debug_box_clearance",
           "mind_forecast_score", "mind_debug_forecast_score",
           "mind_audit_road_plan", "mind_audit_road_episode", "mind_debug_road_margin",
           "mind_audit_ttc", "mind_debug_box_ttc",
           "mind_audit_lane_plan", "mind_audit_lane_episode", "mind_debug_lane_project",
           "mind_loop_create", "mind_loop_destroy", "mind_loop_reset", "mind_loop_advance", "mind_loop_state", "mind_loop_last_plan", "mind_loop_export",
           "mind_planner_create", "mind_planner_destroy", "mind_planner_reset", "mind_planner_observe", "mind_planner_set_lanes", "mind_planner_set_target_lane",
           "mind_planner_set_solve_lane", "mind_planner_set_eval_lane", "mind_planner_plan", "mind_planner_last_plan", "mind_planner_export"]

# transport of the sharded mind_aime_plan (include/mind_hip.h): int fn(void *user, int op, void *send, void *recv, int64 bytes)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
XCHG_ALLGATHER, XCHG_ALLREDUCE, XCHG_ALLTOALLV = 0, 1, 2

_lib = None


def load():
    """Load the library (raises if it has not been built: run ``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: the HIP extension must be built (hipcc --offload-arch=gfx950); "
                          "there is no CPU fallback for the product path")
    lib = C.CDLL(LIB_PATH)
    lib.mind_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.mind_ctx_destroy.argtypes = [C.c_void_p]
    lib.mind_last_error_string.argtypes = [C.c_void_p]
    lib.mind_last_error_string.restype = C.c_char_p
    lib.mind_ctx_synchronize.argtypes = [C.c_void_p]
    lib.mind_weights_load.argtypes = [C.c_void_p, C.POINTER(TensorDesc), C.c_int]
    lib.mind_predict_batch.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(PredOut)]
    lib.mind_predict_batch_aux.argtypes = [C.c_void_p, C.POINTER(SceneBatch), C.POINTER(PredOut), C.POINTER(PredAux)]
    lib.mind_set_decoder_basis.argtypes = [C.c_void_p, C.c_int]
    lib.mind_get_decoder_basis.argtypes = [C.c_void_p]
    lib.mind_curve_eval.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_debug_curve_basis.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mind_last_fusion_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)]
    lib.mind_last_actor_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.mind_debug_actor_lw_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]
    lib.mind_last_token_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.mind_last_token_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    lib.mind_debug_token_lw_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong)]
    lib.mind_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.mind_debug_launch_times.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mind_debug_launch_clock.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_ulonglong), C.c_longlong,
                                            C.POINTER(C.c_double), C.c_int]
    lib.mind_ilqr_solve_trees.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(CostTree), C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(IlqrStats)]
    lib.mind_ilqr_contingency.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(IlqrCfg), C.POINTER(CostTree), C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(IlqrStats), C.POINTER(IlqrStats)]
    lib.mind_ilqr_contingency_begin.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(IlqrCfg), C.POINTER(CostTree), C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(IlqrStats), C.POINTER(IlqrStats)]
    lib.mind_ilqr_finish.argtypes = [C.c_void_p]
    lib.mind_ilqr_contingency_begin_plan.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(IlqrCfg), C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_fill_tracks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_ilqr_solve_fields.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(FieldGrid), C.POINTER(CostTree), C.c_int,
                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(IlqrStats)]
    lib.mind_cost_eval.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(FieldGrid), C.POINTER(CostTree),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int, C.c_int,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mind_ilqr_score_trees.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(FieldGrid), C.POINTER(CostTree), C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int, C.c_int,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mind_ilqr_gains.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(FieldGrid), C.POINTER(CostTree), C.c_int,
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int,
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(IlqrGainsOut)]
    lib.mind_ilqr_policy_rollouts.argtypes = [C.c_void_p, C.POINTER(IlqrCfg), C.POINTER(FieldGrid), C.POINTER(CostTree), C.c_int,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.mind_lane_dist_field.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int,
                                         C.c_double] + [C.POINTER(C.c_double)] * 4
    lib.mind_aime_world.argtypes = [C.c_void_p, C.POINTER(WorldIn), C.POINTER(WorldOut)]
    lib.mind_aime_rebase.argtypes = [C.c_void_p, C.POINTER(RebaseIn), C.POINTER(RebaseOut)]
    lib.mind_debug_aime_decide.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_float), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_aime_plan.argtypes = [C.c_void_p, C.POINTER(AimePlanIn), C.POINTER(AimePlanOut)]
    lib.mind_aime_plan_begin.argtypes = [C.c_void_p, C.POINTER(AimePlanIn)]
    lib.mind_aime_plan_poll.argtypes = [C.c_void_p]
    lib.mind_aime_plan_finish.argtypes = [C.c_void_p, C.POINTER(AimePlanOut)]
    lib.mind_ctx_busy.argtypes = [C.c_void_p]
    lib.mind_ilqr_finish_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_set_pair_precision.argtypes = [C.c_void_p, C.c_int]
    lib.mind_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.mind_get_tuning.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.mind_debug_tuning.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_int)]
    lib.mind_debug_live_handles.argtypes = []
    lib.mind_last_ilqr_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mind_last_ilqr_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.mind_last_ilqr_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    lib.mind_eval_traj_trees.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_double, C.POINTER(C.c_double)]
    lib.mind_get_pair_precision.argtypes = [C.c_void_p]
    lib.mind_debug_pack_bfrag.argtypes = [C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_uint32)]
    lib.mind_debug_pair_schedule.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    lib.mind_debug_predict_choice.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                              C.c_int, C.POINTER(C.c_longlong), C.c_int]
    lib.mind_debug_ilqr_plan.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_int)]
    lib.mind_debug_wait_word.argtypes = [C.POINTER(C.c_uint), C.c_uint, C.c_double, WAIT_CLOCK, C.c_void_p, C.c_int]
    lib.mind_debug_aime_book.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_int), C.POINTER(C.c_float)] + [C.c_int] * 4 + [C.POINTER(C.c_longlong), C.c_int, C.c_char_p, C.c_int]
    lib.mind_debug_trig.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    lib.mind_debug_pack_conv_frag.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_size_t]
    lib.mind_debug_pack.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    lib.mind_debug_weight_image.argtypes = [C.POINTER(TensorDesc), C.c_int, C.POINTER(C.c_float), C.c_size_t, C.c_char_p, C.c_size_t,
                                            C.POINTER(C.c_longlong), C.c_int, C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    lib.mind_debug_weight_bind.argtypes = [C.POINTER(TensorDesc), C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    lib.mind_debug_dec_scene.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_float)]
    lib.mind_debug_set_layers.argtypes = [C.c_void_p, C.c_int]
    lib.mind_debug_token_form.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.mind_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_float), C.c_int64]
    lib.mind_set_exchange.argtypes = [C.c_void_p, C.c_int, C.c_int, EXCHANGE_FN, C.c_void_p, C.c_int]
    lib.mind_last_exchange_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.mind_loop_create.argtypes = [C.c_void_p, C.POINTER(LoopDesc), C.POINTER(C.c_void_p)]
    lib.mind_loop_destroy.argtypes = [C.c_void_p]
    lib.mind_loop_reset.argtypes = [C.c_void_p]
    lib.mind_loop_advance.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_longlong, C.POINTER(LoopOut)]
    lib.mind_loop_state.argtypes = [C.c_void_p, C.POINTER(LoopOut)]
    lib.mind_loop_last_plan.argtypes = [C.c_void_p, C.POINTER(AimePlanOut)] + [C.POINTER(C.c_void_p)] * 6 + [C.c_void_p]
    lib.mind_loop_export.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_planner_create.argtypes = [C.c_void_p, C.POINTER(PlannerDesc), C.POINTER(C.c_void_p)]
    lib.mind_planner_destroy.argtypes = [C.c_void_p]
    lib.mind_planner_reset.argtypes = [C.c_void_p]
    lib.mind_planner_observe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_planner_set_lanes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mind_planner_set_target_lane.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mind_planner_set_solve_lane.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_double]
    lib.mind_planner_set_eval_lane.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.mind_planner_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PlannerOut)]
    lib.mind_planner_last_plan.argtypes = [C.c_void_p, C.POINTER(AimePlanOut)] + [C.POINTER(C.c_void_p)] * 6 + [C.c_void_p]
    lib.mind_planner_export.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mind_audit_plan.argtypes = [C.c_void_p, C.POINTER(AuditBox), C.c_double, C.POINTER(CostTree), C.c_int, C.c_int, C.POINTER(C.c_double),
                                    C.POINTER(AuditPlanOut)]
    lib.mind_audit_episode.argtypes = [C.c_void_p, C.POINTER(AuditBox), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(AuditEpisodeOut)]
    lib.mind_debug_box_clearance.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    fc_tail = [C.POINTER(ForecastCfg), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8),
               C.POINTER(C.c_uint8), C.POINTER(ForecastOut)]
    lib.mind_forecast_score.argtypes = [C.c_void_p] + fc_tail
    lib.mind_debug_forecast_score.argtypes = fc_tail
    road = [C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]
    lib.mind_audit_road_plan.argtypes = [C.c_void_p, C.POINTER(AuditBox)] + road + [C.POINTER(CostTree), C.c_int, C.c_int, C.POINTER(C.c_double),
                                                                                   C.POINTER(AuditRoadPlanOut)]
    lib.mind_audit_road_episode.argtypes = [C.c_void_p, C.POINTER(AuditBox)] + road + [C.c_int, C.c_int, C.POINTER(C.c_double),
                                                                                      C.POINTER(AuditRoadEpisodeOut)]
    lib.mind_debug_road_margin.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(AuditBox)] + road + [C.POINTER(C.c_double), C.POINTER(C.c_double)] + \
        [C.POINTER(C.c_int32)] * 3
    lib.mind_audit_ttc.argtypes = [C.c_void_p, C.POINTER(AuditBox), C.POINTER(AuditTtcCfg), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(AuditTtcOut)]
    lib.mind_debug_box_ttc.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lanes = [C.POINTER(AuditBox), C.POINTER(AuditLaneCfg), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]
    lib.mind_audit_lane_plan.argtypes = [C.c_void_p] + lanes + [C.POINTER(CostTree), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(AuditLanePlanOut)]
    lib.mind_audit_lane_episode.argtypes = [C.c_void_p] + lanes + [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(AuditLaneEpisodeOut)]
    lib.mind_debug_lane_project.argtypes = [C.c_int, C.POINTER(C.c_double)] + lanes + [C.POINTER(C.c_double)] * 5 + [C.POINTER(C.c_int32)] * 2 + \
        [C.POINTER(C.c_double)]
    for n in EXPORTS:
        getattr(lib, n)
        if n not in ("mind_last_error_string", "mind_debug_read"):
            getattr(lib, n).restype = C.c_int
    lib.mind_debug_read.restype = C.c_int64
    _lib = lib
    return lib


# header of mind_debug_predict_choice's record (include/mind_hip.h)
PRED_CHOICE_FIELDS = ("header", "n_runs", "np", "actor_form", "actor_arg", "actor_grid", "actor_chunk", "actor_chunks", "actor_launches", "qsplit", "qk_stride",
                      "tiled", "edge_bf16", "edge_pair_bytes", "tok_chunk", "tok_lw", "tok_chunks", "pair_family", "pair_np", "l5_jobs5", "xcd_lanes",
                      "xcd_lanes5", "dec_actor", "dec_np", "fp32_dec", "split_dec", "want_mw", "mw_blocks", "cls_on_side", "tgt_wait_first",
                      "dec_head_ra", "dec_chain_g")
PAIR_PREC = ("f32", "bf16x3", "bf16", "bf16x6")


def predict_choice(knobs, prec, scenes, n_cu=256, have_side=True):
    """pred_choose's record (mind_debug_predict_choice; no GPU) for mind_set_tuning pairs `knobs`, the arithmetic `prec` (name or 0..3) and
    scenes [(actors, lanes), ...]: dict of PRED_CHOICE_FIELDS + "runs" = [(t0, n, kind, layerwise, small, merged), ...]; None when rejected"""
    lib = load()
    names = (C.c_char_p * max(1, len(knobs)))(*[k.encode() for k in knobs])
    vals = (C.c_int * max(1, len(knobs)))(*[int(v) for v in knobs.values()])
    sa = (C.c_int * len(scenes))(*[a for a, _ in scenes])
    sl = (C.c_int * len(scenes))(*[l for _, l in scenes])
    cap = 32 + 6 * len(scenes)
    out = (C.c_longlong * cap)()
    n = lib.mind_debug_predict_choice(names, vals, len(knobs), PAIR_PREC.index(prec) if isinstance(prec, str) else prec, n_cu, int(have_side),
                                      sa, sl, len(scenes), out, cap)
    if n == MIND_EINVAL:
        return None
    assert 0 < n <= cap and out[0] == 32 and n == 32 + 6 * out[1], n
    d = dict(zip(PRED_CHOICE_FIELDS, out[:32]))
    d["runs"] = [tuple(out[32 + 6 * i:38 + 6 * i]) for i in range(out[1])]
    return d


TOKEN_FORMS = ("rule", "k_token_m", "k_token_s<4>", "k_token_s<2>")


def token_form(form, n_tok=0, n_cu=256, ctx=None):
    """mind_debug_token_form: the kernel (index into TOKEN_FORMS; 0: its run is not small and merged) of a lone scene of n_tok tokens on n_cu CUs
    under `form` (0 the rule); with a context, `form` holds for the context's later calls.  None when rejected.  No GPU without a context."""
    n = load().mind_debug_token_form(ctx, int(form), int(n_tok), int(n_cu))
    return None if n == MIND_EINVAL else n


def dec_scene(lib, ctx, rows, form, reps=1, timed=False):
    """mind_debug_dec_scene: the decoder's scene part alone on the cls token rows `rows` [B,128] in form 0 (k_dec_scene) or 8 / 16 / 32 (the launch
    chain with that many workgroups per scene) -> (Cout [B,6,128], cls [B,6]) and, if timed, the milliseconds of each of the reps repetitions"""
    import numpy as np
    rows = np.ascontiguousarray(rows, np.float32)
    B = rows.shape[0]
    assert rows.shape == (B, 128)
    fp = C.POINTER(C.c_float)
    cout, cls, ms = np.empty((B, 6, 128), np.float32), np.empty((B, 6), np.float32), np.zeros(reps, np.float32)
    check(lib, ctx, lib.mind_debug_dec_scene(ctx, rows.ctypes.data_as(fp), B, int(form), cout.ctypes.data_as(fp), cls.ctypes.data_as(fp), reps,
                                             ms.ctypes.data_as(fp) if timed else None), "mind_debug_dec_scene")
    return (cout, cls, ms) if timed else (cout, cls)


def knobs():
    """the knob table (mind_debug_tuning; no GPU), in its order: [(mind_set_tuning name, environment variable or None, default), ...]"""
    lib = load()
    name, env, val = C.c_char_p(), C.c_char_p(), C.c_int()
    rows = []
    while not rows or len(rows) < n:
        n = lib.mind_debug_tuning(len(rows), None, None, 0, C.byref(name), C.byref(env), C.byref(val))
        assert n > 0, n
        rows.append((name.value.decode(), env.value.decode() if env.value else None, val.value))
    return rows


def knob_stored(name, value=None, text=None):
    """what a fresh record stores for knob `name` after mind_set_tuning(name, value), or after its variable was read with `text` (no GPU);
    None when the library rejects the name, or the text of a knob without a variable"""
    val = C.c_int()
    rc = load().mind_debug_tuning(-1, name.encode(), None if text is None else text.encode(), 0 if value is None else int(value), None, None, C.byref(val))
    return val.value if rc == MIND_OK else None


# header and per-tree tables of mind_debug_ilqr_plan's record (include/mind_hip.h)
ILQR_PLAN_FIELDS = ("header", "n_trees", "form", "G", "GS", "spec", "nslot", "grid", "workgroups_per_tree", "host_out", "early", "starve_followers")
ILQR_TREE_FIELDS = ("M", "nl", "nseg", "nsl", "maxls", "nfs")
ILQR_TREE_TABLES = ("level_start", "level_nodes", "child_start", "child_list", "seg_start", "seg_nodes", "slevel_start", "slevel_segs", "seg_rec",
                    "fstep_start", "fstep_items", "fstep_q1", "fstep_nstart", "fstep_nodes")


def ilqr_plan(knobs, parents, n_cu=256, generic=False, evaluate=False, two_fits=False):
    """il_choose's record and il_tree_tables' tables (mind_debug_ilqr_plan; no GPU) for mind_set_tuning pairs `knobs` and the cost trees whose
    parent arrays are `parents`: dict of ILQR_PLAN_FIELDS + "trees" = [dict of ILQR_TREE_FIELDS and ILQR_TREE_TABLES (lists of ints), ...];
    {"bad": (tree, node)} for a node whose parent is not below it; None when rejected otherwise"""
    lib = load()
    names = (C.c_char_p * max(1, len(knobs)))(*[k.encode() for k in knobs])
    vals = (C.c_int * max(1, len(knobs)))(*[int(v) for v in knobs.values()])
    nn = (C.c_int * len(parents))(*[len(p) for p in parents])
    flat = [int(v) for p in parents for v in p]
    par = (C.c_int32 * max(1, len(flat)))(*flat)
    bad = (C.c_int * 2)()
    mode = int(generic) | int(evaluate) << 1 | int(two_fits) << 2
    n = lib.mind_debug_ilqr_plan(names, vals, len(knobs), n_cu, mode, len(parents), nn, par, None, 0, bad)
    if n == MIND_EINVAL:
        return {"bad": (bad[0], bad[1])} if bad[0] >= 0 else None
    out = (C.c_longlong * n)()
    assert lib.mind_debug_ilqr_plan(names, vals, len(knobs), n_cu, mode, len(parents), nn, par, out, n, bad) == n and out[0] == 16
    d = dict(zip(ILQR_PLAN_FIELDS, out[:12]))
    d["trees"], o = [], 16
    for _ in parents:
        tr = dict(zip(ILQR_TREE_FIELDS, out[o:o + 6]))
        lens, o = out[o + 6:o + 20], o + 20
        for name, ln in zip(ILQR_TREE_TABLES, lens):
            tr[name], o = list(out[o:o + ln]), o + ln
        d["trees"].append(tr)
    assert o == n
    return d


AIME_ROUND_FIELDS = ("B", "lo", "hi", "Bmax", "chunk", "S", "s0", "Sm", "any")
AIME_NODE_FIELDS = ("round", "scene", "mode", "parent", "prob", "cur_t", "end_t", "flags", "dur", "row_off", "owner", "lscene")


def aime_book(pred_len, max_depth, n_agents, rounds, world=1, rank=0, force=False, max_rounds=32, n_tokens=0, bytes_per_pair=512, plan_chunk_mb=96 * 1024,
              per_scene=1):
    """mind_aime_plan's bookkeeping (mind_debug_aime_book; no GPU) replayed over `rounds`, one float32 array of decision words per round
    ([ranks, 24 * Bmax]: sel | sel_prob | hit, include/mind_hip.h).  -> dict: "error" (None or the plan's message), "code", "rounds" = [dict of
    AIME_ROUND_FIELDS + todo, cnt_r, s0_r, win, tab, snd, rcv], and without an error "nodes" (dicts of AIME_NODE_FIELDS, prob as float32 bits),
    "gather" / "flat" (jobs [(row0, n, dst, a, round)], job_of_block, agent_of_block, bytes), tree_top, tree_off, flat_parent, flat_prob
    (float32 bits), n_rows, root_flags; None when the arguments are rejected"""
    import numpy as np
    lib = load()
    arrs = [np.ascontiguousarray(r, np.float32).ravel() for r in rounds]
    lens = (C.c_int * max(1, len(arrs)))(*[a.size for a in arrs])
    dec = np.concatenate(arrs + [np.zeros(1, np.float32)])
    msg = C.create_string_buffer(256)
    args = [pred_len, max_depth, max_rounds, n_agents, world, rank, int(force), len(arrs), lens, dec.ctypes.data_as(C.POINTER(C.c_float)), n_tokens,
            bytes_per_pair, plan_chunk_mb, per_scene]
    n = lib.mind_debug_aime_book(*args, None, 0, msg, 256)
    if n == MIND_EINVAL:
        return None
    out = (C.c_longlong * n)()
    assert lib.mind_debug_aime_book(*args, out, n, msg, 256) == n and out[0] == 16
    o, take = [16], lambda k: (list(out[o[0]:o[0] + k]), o.__setitem__(0, o[0] + k))[0]
    d = dict(code=out[1], error=msg.value.decode() if out[1] else None, args=(out[2], out[3]), n_rows=out[8], root_flags=out[9], rounds=[])
    for _ in range(out[4]):
        r = dict(zip(AIME_ROUND_FIELDS, take(9)))
        for k, ln in (("todo", r["S"]), ("cnt_r", world), ("s0_r", world + 1), ("win", 3 * r["Sm"]), ("tab", 2 * world), ("snd", 2 * world), ("rcv", 2 * world)):
            r[k] = take(ln)
        d["rounds"].append(r)
    if not out[1]:
        d["nodes"] = [dict(zip(AIME_NODE_FIELDS, take(12))) for _ in range(out[5])]
        for name in ("gather", "flat"):
            nj, nb, nbytes = take(3)
            d[name] = dict(jobs=[tuple(take(5)) for _ in range(nj)], job_of_block=take(nb), agent_of_block=take(nb), bytes=nbytes)
        d["tree_top"], d["tree_off"], d["flat_parent"], d["flat_prob"] = take(out[6]), take(out[6] + 1), take(out[7]), take(out[7])
    assert o[0] == n
    return d


def tensor_descs(sd):
    """(TensorDesc array, the float32 arrays it points into -- keep them alive while it is used) of a state_dict of arrays or torch tensors"""
    import numpy as np
    descs = (TensorDesc * max(1, len(sd)))()
    keep = []
    for i, (k, v) in enumerate(sd.items()):
        a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), dtype=np.float32)
        keep.append(a)
        descs[i].name = k.encode()
        descs[i].data = a.ctypes.data_as(C.POINTER(C.c_float))
        descs[i].numel = a.size
    return descs, keep


def weight_image(sd):
    """wp_pack's blob of a state_dict (mind_debug_weight_image; no GPU) -> (float32 blob, [(entry key, offset, length in floats), ...] in blob
    order); raises KeyError naming the tensor that is missing or has the wrong size"""
    import numpy as np
    lib = load()
    descs, keep = tensor_descs(sd)
    msg = C.create_string_buffer(256)
    info = (C.c_longlong * 3)()
    rc = lib.mind_debug_weight_image(descs, len(sd), None, 0, None, 0, None, 0, info, msg, 256)        # the sizes
    if rc == MIND_ENOTFOUND:
        raise KeyError(msg.value.decode())
    assert rc == MIND_OK, rc
    ne, nf, nb = info
    blob, names, ents = np.zeros(nf, np.float32), C.create_string_buffer(nb), (C.c_longlong * (2 * ne))()
    assert lib.mind_debug_weight_image(descs, len(sd), blob.ctypes.data_as(C.POINTER(C.c_float)), nf, names, nb, ents, ne, info, msg, 256) == MIND_OK
    keys = names.value.decode().split("\n")[:-1]
    assert len(keys) == ne
    return blob, [(k, ents[2 * i], ents[2 * i + 1]) for i, k in enumerate(keys)]


def curve_basis(basis, tau):
    """the basis rows mind_curve_eval evaluates for the times `tau` (mind_debug_curve_basis; no GPU): (T [n,8], Tp [n,7]) float32; `basis` a
    name of BASIS or its number.  Raises ValueError for what the library rejects (a tau outside [0, 1] or not finite, no tau, an unknown basis)"""
    import numpy as np
    lib = load()
    tau = np.ascontiguousarray(tau, np.float64).ravel()
    b = BASIS.index(basis) if isinstance(basis, str) else int(basis)
    T, Tp = np.zeros((max(1, tau.size), 8), np.float32), np.zeros((max(1, tau.size), 7), np.float32)
    rc = lib.mind_debug_curve_basis(b, tau.ctypes.data_as(C.POINTER(C.c_double)), tau.size, T.ctypes.data_as(C.POINTER(C.c_float)),
                                    Tp.ctypes.data_as(C.POINTER(C.c_float)))
    if rc == MIND_EINVAL:
        raise ValueError(f"mind_debug_curve_basis rejects basis {basis!r}, tau {tau!r}")
    assert rc == MIND_OK, rc
    return T[:tau.size], Tp[:tau.size]


def weight_bind(sd, drop=None):
    """wp_pack + wp_bind against the host image (mind_debug_weight_bind; no GPU) with the blob entry `drop` forgotten in between -> None when
    every required entry is bound, else the name of the first missing one (a state_dict tensor when packing fails, a blob key when binding does)"""
    lib = load()
    descs, keep = tensor_descs(sd)
    msg = C.create_string_buffer(256)
    rc = lib.mind_debug_weight_bind(descs, len(sd), drop.encode() if drop else None, msg, 256)
    assert rc in (MIND_OK, MIND_ENOTFOUND), rc
    return None if rc == MIND_OK else msg.value.decode()


def pack(what, w, a=0, b=0, c=0, cap=1 << 20):
    """one packer of weight_pack.h by name (mind_debug_pack; no GPU): float32 array in -> float32 array out (bf16 fragments: view as uint32)"""
    import numpy as np
    lib = load()
    w = np.ascontiguousarray(w, np.float32)
    out = np.zeros(cap, np.float32)
    n = lib.mind_debug_pack(what.encode(), w.ctypes.data_as(C.POINTER(C.c_float)), a, b, c, out.ctypes.data_as(C.POINTER(C.c_float)), cap)
    assert n > 0, (what, n)
    return out[:n].copy()


def box_clearance(kind, a, b, trig=None):
    """box_geom.h on the CPU (mind_debug_box_clearance; no GPU), pair by pair: a [n, 5] = (x, y, yaw, L, W) against b [n, 5] -- kind 0 (or
    "disc"): discs (x, y, r, -, -), kind 1 (or "rect"): rectangles; trig [n, 4] = (cos a, sin a, cos b, sin b), None = the kernels' own
    sin / cos.  -> float64 [n]"""
    import numpy as np
    lib = load()
    kind = {"disc": 0, "rect": 1}.get(kind, kind)
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 5)
    b = np.ascontiguousarray(b, np.float64).reshape(-1, 5)
    tg = None if trig is None else np.ascontiguousarray(trig, np.float64).reshape(-1, 4)
    if len(b) != len(a) or (tg is not None and len(tg) != len(a)):
        raise ValueError(f"box_clearance: {len(a)} boxes a, {len(b)} b" + ("" if tg is None else f", {len(tg)} trig rows"))
    out = np.zeros(len(a))
    dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.mind_debug_box_clearance(int(kind), len(a), dp(a), dp(b), dp(tg), dp(out))
    if rc != MIND_OK:
        raise ValueError(f"mind_debug_box_clearance rejects kind {kind!r}")
    return out


def box_ttc(a, b, trig=None):
    """ttc_geom.h on the CPU (mind_debug_box_ttc; no GPU), pair by pair: the first time at which the rectangles a [n, 7] = (x, y, yaw, L, W,
    vx, vy) and b [n, 7], each translating at its constant velocity, overlap -- 0.0 when they do now, +inf when they never do; touching is
    no hit, and there is no horizon.  trig [n, 4] = (cos a, sin a, cos b, sin b), None = the kernels' own sin / cos.  -> float64 [n]"""
    import numpy as np
    lib = load()
    a = np.ascontiguousarray(a, np.float64).reshape(-1, 7)
    b = np.ascontiguousarray(b, np.float64).reshape(-1, 7)
    tg = None if trig is None else np.ascontiguousarray(trig, np.float64).reshape(-1, 4)
    if len(b) != len(a) or (tg is not None and len(tg) != len(a)):
        raise ValueError(f"box_ttc: {len(a)} boxes a, {len(b)} b" + ("" if tg is None else f", {len(tg)} trig rows"))
    out = np.zeros(len(a))
    dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.mind_debug_box_ttc(len(a), dp(a), dp(b), dp(tg), dp(out))
    if rc != MIND_OK:
        raise ValueError(f"mind_debug_box_ttc rejects its arguments ({rc})")
    return out


def audit_box(box, name="ego_box"):
    """(length, width[, center_offset]) -> mind_audit_box"""
    import numpy as np
    b = np.asarray(box, np.float64).ravel()
    if b.size not in (2, 3) or not np.all(np.isfinite(b)) or np.any(b[:2] < 0.0):
        raise ValueError(f"{name} must be (length, width[, center_offset]) with finite length, width >= 0, got {box!r}")
    return AuditBox(float(b[0]), float(b[1]), float(b[2]) if b.size == 3 else 0.0)


def road_args(verts, poly_off):
    """a road as the C entries take it: (verts float64 [V, 2], poly_off int32 [P + 1], their pointers, P); the shapes are checked here, the
    road's own rules (three vertices per ring, finite, ascending) by the library"""
    import numpy as np
    v = np.ascontiguousarray(verts, np.float64)
    off = np.ascontiguousarray(poly_off, np.int32).ravel()
    if v.ndim != 2 or v.shape[1] != 2 or off.size < 2 or int(off[-1]) != len(v):
        raise ValueError(f"a road is verts [V, 2] and poly_off [P + 1] ending in V, got {list(v.shape)} and poly_off {off.tolist()[:8]}")
    return v, off, v.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int32)), off.size - 1


def road_margin(boxes, ego_box, verts, poly_off, trig=None):
    """road_geom.h on the CPU (mind_debug_road_margin; no GPU): boxes [n, 3] = (x, y, yaw) of the box ``ego_box`` = (length, width[,
    center_offset]) against the road verts [V, 2] / poly_off [P + 1]; trig [n, 2] = (cos, sin), None = the kernels' own sin / cos.
    -> dict margin float64 [n], corner, ring, edge int32 [n]"""
    import numpy as np
    lib = load()
    b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 3)
    tg = None if trig is None else np.ascontiguousarray(trig, np.float64).reshape(-1, 2)
    if tg is not None and len(tg) != len(b):
        raise ValueError(f"road_margin: {len(b)} boxes, {len(tg)} trig rows")
    v, off, vp, op, P = road_args(verts, poly_off)
    res = dict(margin=np.zeros(len(b)), corner=np.zeros(len(b), np.int32), ring=np.zeros(len(b), np.int32), edge=np.zeros(len(b), np.int32))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    box = audit_box(ego_box)
    rc = lib.mind_debug_road_margin(len(b), dp(b), C.byref(box), vp, op, P, dp(tg), dp(res["margin"]), ip(res["corner"]), ip(res["ring"]), ip(res["edge"]))
    if rc != MIND_OK:
        raise ValueError(f"mind_debug_road_margin rejects its arguments ({rc}): a ring needs three vertices, poly_off must start at 0 and ascend, "
                         "vertices must be finite")
    return res


LANE_KEYS = ("lat", "s", "along", "across", "lane", "edge")      # the per-box outputs of the lane audit, [2, n] each: 0 = any, 1 = with the flow


def lane_args(verts, lane_off):
    """lanes as the C entries take them: (verts float64 [V, 2], lane_off int32 [P + 1], their pointers, P); the shapes are checked here, the
    lanes' own rules (two vertices per lane, finite, ascending) by the library"""
    import numpy as np
    v = np.ascontiguousarray(verts, np.float64)
    off = np.ascontiguousarray(lane_off, np.int32).ravel()
    if v.ndim != 2 or v.shape[1] != 2 or off.size < 2 or int(off[-1]) != len(v):
        raise ValueError(f"lanes are verts [V, 2] and lane_off [P + 1] ending in V, got {list(v.shape)} and lane_off {off.tolist()[:8]}")
    return v, off, v.ctypes.data_as(C.POINTER(C.c_double)), off.ctypes.data_as(C.POINTER(C.c_int32)), off.size - 1


def lane_cfg(cos_flow, bound, form=0):
    """-> mind_audit_lane_cfg, checked as the library checks it"""
    import numpy as np
    cos_flow, bound = float(cos_flow), float(bound)
    if not -1.0 <= cos_flow <= 1.0:
        raise ValueError(f"cos_flow must lie in [-1, 1], got {cos_flow!r}")
    if not np.isfinite(bound) or bound <= 0.0:
        raise ValueError(f"bound must be finite and > 0, got {bound!r}")
    if form not in (0, 1, 2):
        raise ValueError(f"form must be 0 (the library's rule), 1 (thread per box) or 2 (one wavefront per box), got {form!r}")
    return AuditLaneCfg(cos_flow, bound, int(form))


def lane_project(boxes, ego_box, verts, lane_off, cos_flow, bound, trig=None):
    """lane_geom.h on the CPU (mind_debug_lane_project; no GPU): the centres of the boxes [n, 3] = (x, y, yaw) of ``ego_box`` = (length,
    width[, center_offset]) against the lanes verts [V, 2] / lane_off [P + 1]; trig [n, 2] = (cos, sin), None = the kernels' own sin / cos.
    -> dict lat, s, along, across float64 [2, n], lane, edge int32 [2, n] (0 = any, 1 = with the flow), margin float64 [n]"""
    import numpy as np
    lib = load()
    b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 3)
    tg = None if trig is None else np.ascontiguousarray(trig, np.float64).reshape(-1, 2)
    if tg is not None and len(tg) != len(b):
        raise ValueError(f"lane_project: {len(b)} boxes, {len(tg)} trig rows")
    v, off, vp, op, P = lane_args(verts, lane_off)
    n = len(b)
    res = {k: np.zeros((2, n), np.int32 if k in ("lane", "edge") else np.float64) for k in LANE_KEYS}
    res["margin"] = np.zeros(n)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    box, cfg = audit_box(ego_box), lane_cfg(cos_flow, bound)
    rc = lib.mind_debug_lane_project(n, dp(b), C.byref(box), C.byref(cfg), vp, op, P, dp(tg), dp(res["lat"]), dp(res["s"]), dp(res["along"]),
                                     dp(res["across"]), ip(res["lane"]), ip(res["edge"]), dp(res["margin"]))
    if rc != MIND_OK:
        raise ValueError(f"mind_debug_lane_project rejects its arguments ({rc}): a lane needs two vertices, lane_off must start at 0 and ascend, "
                         "vertices must be finite")
    return res


def out_record(rec, shape_of, want=None):
    """A record of optional output pointers (mind_audit_*_out, mind_forecast_out) over freshly allocated result arrays: every field of
    the ctypes record ``rec`` that ``want`` names (None = all) gets a zeroed array of shape ``shape_of(name)`` and of the element type its
    pointer declares; the others stay null.  -> (record, results by name in field order)"""
    import numpy as np
    out, res = rec(), {}
    dtype = {C.c_double: np.float64, C.c_int32: np.int32}
    for name, ptr in rec._fields_:
        if want is None or name in want:
            res[name] = np.zeros(shape_of(name), dtype[ptr._type_])
            setattr(out, name, res[name].ctypes.data_as(ptr))
    return out, res


def forecast_args(K, T, actor_off, gt, valid, scored, horizons, miss_radius, disc_scale, disc_offset, want=None):
    """The host-side arguments of mind_forecast_score / mind_debug_forecast_score: checked numpy arrays, the configuration and the output
    record over freshly allocated result arrays (``want``: names of mind_forecast_out, None = all).  -> (cfg, B, actor_off, gt, valid,
    scored, out, results, keep)"""
    import numpy as np
    off = np.ascontiguousarray(actor_off, np.int32).ravel()
    if off.size < 1:
        raise ValueError("actor_off must hold B + 1 offsets")
    B, A = off.size - 1, int(off[-1])
    g = np.ascontiguousarray(gt, np.float64)
    v = np.ascontiguousarray(valid, np.uint8)
    if g.shape != (A, T, 2) or v.shape != (A, T):
        raise ValueError(f"gt must be [{A}, {T}, 2] and valid [{A}, {T}], got {list(g.shape)} and {list(v.shape)}")
    sc = None if scored is None else np.ascontiguousarray(scored, np.uint8)
    if sc is not None and sc.shape != (A,):
        raise ValueError(f"scored must be [{A}], got {list(sc.shape)}")
    hz = np.ascontiguousarray(horizons, np.int32).ravel()
    cfg = ForecastCfg(int(K), int(T), int(hz.size), hz.ctypes.data_as(C.POINTER(C.c_int32)), float(miss_radius), float(disc_scale), float(disc_offset))
    names = [n for n, _, _, _ in FORECAST_OUT]
    if want is not None and any(n not in names for n in want):
        raise ValueError(f"forecast outputs are {names}, got {list(want)}")
    shape = {n: (A if per == "a" else B, hz.size) + ((int(K),) if has_k else ()) for n, _, per, has_k in FORECAST_OUT}
    out, res = out_record(ForecastOut, shape.__getitem__, want)
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    return (cfg, B, off.ctypes.data_as(C.POINTER(C.c_int32)), g.ctypes.data_as(C.POINTER(C.c_double)), u8(v), u8(sc), out, res, (off, g, v, sc, hz))


def forecast_gather(res):
    """the conveniences min_ade, min_fde [A, n_h] and s_min_ade, s_min_fde [B, n_h]: the values at the arg-minima (NaN for -1)"""
    import numpy as np
    for pre in ("", "s_"):
        for m in ("ade", "fde"):
            v, k = res.get(pre + m), res.get(pre + "k_" + m)
            if v is not None and k is not None:
                g = np.take_along_axis(v, np.maximum(k, 0)[..., None], axis=-1)[..., 0] if v.size else np.zeros(k.shape)
                res[pre + "min_" + m] = np.where(k >= 0, g, np.nan)
    return res


def forecast_score_host(reg, cls, actor_off, gt, valid, scored=None, horizons=(60,), miss_radius=2.0, disc_scale=1.0, disc_offset=0.0, want=None):
    """forecast_score.h on the CPU (mind_debug_forecast_score; no GPU): reg [A, K, T, 5] / cls [B, K] float32 host arrays, the rest as
    HipPredictor.forecast_score takes it.  -> the same dict of numpy arrays"""
    import numpy as np
    lib = load()
    r = np.ascontiguousarray(reg, np.float32)
    c = np.ascontiguousarray(cls, np.float32)
    if r.ndim != 4 or r.shape[3] != 5 or c.ndim != 2 or c.shape[1] != r.shape[1]:
        raise ValueError(f"reg must be [A, K, T, 5] and cls [B, K], got {list(r.shape)} and {list(c.shape)}")
    K, T = r.shape[1], r.shape[2]
    cfg, B, off, g, v, sc, out, res, keep = forecast_args(K, T, actor_off, gt, valid, scored, horizons, miss_radius, disc_scale, disc_offset, want)
    if r.shape[0] != keep[0][-1] or c.shape[0] != B:
        raise ValueError(f"reg holds {r.shape[0]} agents and cls {c.shape[0]} scenes, actor_off says {int(keep[0][-1])} and {B}")
    rc = lib.mind_debug_forecast_score(C.byref(cfg), B, off, C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data), g, v, sc, C.byref(out))
    if rc != MIND_OK:
        raise ValueError(f"mind_debug_forecast_score rejects its arguments ({rc})")
    return forecast_gather(res)


class MindError(RuntimeError):
    pass


def check(lib, ctx, rc, what):
    if rc != MIND_OK:
        msg = lib.mind_last_error_string(ctx) if ctx else b""
        raise MindError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
