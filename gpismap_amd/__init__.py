"""gpismap_amd -- MI355X-native GPisMap hot path (ObsGP + OnGPIS on hand-written HIP kernels).

Thin ctypes binding of the C-ABI in include/gpismap_amd.h.  The classes mirror the command set of
the reference's mex gateways (mex/mexGPisMap3.cpp: 'setCamera' / 'update' / 'test' /
'getAllPoints' / 'reset').  There is NO CPU fallback: if libgpismap_amd.so is missing, or no HIP
device is present, the compute entry points raise.
"""
import ctypes as C
import math
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPISMAP_AMD_LIB", os.path.join(_HERE, "libgpismap_amd.so"))
_lib = None

fp = C.POINTER(C.c_float)
ip = C.POINTER(C.c_int)
dp = C.POINTER(C.c_double)


class GpisError(RuntimeError):
    pass


class gpis_cam(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int), ("height", C.c_int)]


class gpis_render_opts(C.Structure):
    _fields_ = [("tnear", C.c_float), ("tfar", C.c_float), ("min_step", C.c_float), ("max_step", C.c_float),
                ("far_step", C.c_float), ("level", C.c_float), ("max_var", C.c_float), ("refine", C.c_int),
                ("max_steps", C.c_int)]


class gpis_render_field_opts(C.Structure):
    _fields_ = [("tnear", C.c_float), ("tfar", C.c_float), ("min_step", C.c_float), ("max_step", C.c_float),
                ("slack", C.c_float), ("refine", C.c_int), ("max_steps", C.c_int)]


class gpis_track_opts(C.Structure):
    _fields_ = [("max_residual", C.c_double), ("huber", C.c_double), ("max_var", C.c_double), ("damping", C.c_double),
                ("eps_t", C.c_double), ("eps_r", C.c_double), ("level", C.c_float), ("stride", C.c_int),
                ("max_iters", C.c_int), ("min_inliers", C.c_int)]


class gpis_locate_opts(C.Structure):
    _fields_ = [("max_residual", C.c_double), ("stride", C.c_int), ("top_k", C.c_int)]


class gpis_pf_opts(C.Structure):
    _fields_ = [("max_residual", C.c_double), ("beta", C.c_double), ("sigma_t", C.c_double * 3), ("sigma_r", C.c_double),
                ("resample_below", C.c_double), ("stride", C.c_int)]


class gpis_mppi_opts(C.Structure):
    _fields_ = [("dt", C.c_double), ("lambda", C.c_double), ("gamma", C.c_double), ("sigma", C.c_double * 4),
                ("umin", C.c_double * 4), ("umax", C.c_double * 4), ("clearance", C.c_double), ("margin", C.c_double),
                ("w_obs", C.c_double), ("w_col", C.c_double), ("w_off", C.c_double), ("w_goal", C.c_double)]


class gpis_obst_opts(C.Structure):
    _fields_ = [("clearance", C.c_double), ("margin", C.c_double), ("w_obs", C.c_double), ("w_col", C.c_double)]


class gpis_retime_opts(C.Structure):
    _fields_ = [("slot", C.c_double), ("max_pause", C.c_int), ("clearance", C.c_double), ("press_on", C.c_int)]


class gpis_plan_opts(C.Structure):
    _fields_ = [("clearance", C.c_float), ("margin", C.c_float), ("gain", C.c_float), ("connectivity", C.c_int),
                ("max_rounds", C.c_int)]


class gpis_tplan_opts(C.Structure):
    _fields_ = [("clearance", C.c_float), ("margin", C.c_float), ("gain", C.c_float), ("connectivity", C.c_int),
                ("slot", C.c_double), ("horizon", C.c_int), ("dyn_clearance", C.c_double), ("wait", C.c_float),
                ("keep_cost", C.c_int)]


class gpis_tpplan_opts(C.Structure):
    _fields_ = [("clearance", C.c_float), ("margin", C.c_float), ("gain", C.c_float), ("turn", C.c_float), ("slot", C.c_double),
                ("horizon", C.c_int), ("dyn_clearance", C.c_double), ("wait", C.c_float), ("keep_cost", C.c_int)]


class gpis_pplan_opts(C.Structure):
    _fields_ = [("clearance", C.c_float), ("margin", C.c_float), ("gain", C.c_float), ("turn", C.c_float), ("max_rounds", C.c_int)]


class gpis_cover_opts(C.Structure):
    _fields_ = [("back_off", C.c_float), ("max_gap", C.c_float), ("clearance", C.c_float), ("min_size", C.c_int),
                ("max_rounds", C.c_int)]


class gpis_detect_opts(C.Structure):
    _fields_ = [("min_dist", C.c_double), ("link", C.c_double), ("pad", C.c_double), ("max_radius", C.c_double),
                ("gate", C.c_double), ("max_speed", C.c_double), ("alpha", C.c_double), ("min_points", C.c_int),
                ("max_missed", C.c_int), ("stride", C.c_int), ("max_rounds", C.c_int)]


class gpis_view_opts(C.Structure):
    _fields_ = [("march", gpis_render_field_opts), ("back_off", C.c_float), ("max_gap", C.c_float), ("miss", C.c_float),
                ("min_dist", C.c_float)]


class gpis_traj_opts(C.Structure):
    _fields_ = [("clearance", C.c_float), ("margin", C.c_float), ("w_smooth", C.c_float), ("w_obs", C.c_float),
                ("rate", C.c_float), ("max_move", C.c_float), ("tol", C.c_float), ("iters", C.c_int), ("sub", C.c_int)]


class gpis_traj_timing_opts(C.Structure):
    _fields_ = [("v_max", C.c_float), ("v_min", C.c_float), ("a_max", C.c_float), ("d_max", C.c_float), ("a_lat", C.c_float),
                ("w_max", C.c_float), ("v_start", C.c_float), ("v_end", C.c_float), ("clearance", C.c_float),
                ("slow_dist", C.c_float)]


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def lib():
    """Load the native library (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GpisError("native library %s not built; run __graft_entry__.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.gpis_device_count.restype = C.c_int
    L.gpis_pool_cache_trim.restype = C.c_ulonglong
    L.gpis_pool_cache_trim.argtypes = []
    L.gpis_version.restype = C.c_char_p
    L.gpis_set_device.argtypes = [C.c_int]
    L.gpis3_device.argtypes = [vp]
    L.gpis3_set_shard.argtypes = [vp, C.c_int, C.c_int]
    L.gpis3_shard_info.argtypes = [vp, ip, C.c_int]
    L.gpis3_shard_bytes.argtypes = [vp, C.c_int]; L.gpis3_shard_bytes.restype = C.c_longlong
    L.gpis3_shard_pack.argtypes = [vp, vp, vp]
    L.gpis3_shard_unpack.argtypes = [vp, C.c_int, vp, vp]
    L.gpis3_shard_finish.argtypes = [vp]
    if hasattr(L, "gpis3_apply_frame"):
        L.gpis3_set_frame_export.argtypes = [vp, C.c_int]
        L.gpis3_frame_record.argtypes = [vp, vp, C.c_longlong]
        L.gpis3_frame_record.restype = C.c_longlong
        L.gpis3_train_deferred.argtypes = [vp]
        L.gpis3_apply_frame.argtypes = [vp, vp, C.c_longlong]
    L.gpis_ongpis_packed_bytes.argtypes = [vp, ip, C.c_int]; L.gpis_ongpis_packed_bytes.restype = C.c_longlong
    L.gpis_ongpis_pack.argtypes = [vp, ip, C.c_int, vp, C.c_longlong, vp]
    L.gpis_ongpis_unpack.argtypes = [vp, vp, C.c_int, C.c_longlong, ip, vp]
    L.gpis2_device.argtypes = [vp]
    L.gpis3_create.restype = vp
    L.gpis3_create.argtypes = [C.POINTER(gpis_cam)]
    L.gpis3_destroy.argtypes = [vp]
    L.gpis3_reset.argtypes = [vp]
    L.gpis3_set_camera.argtypes = [vp, C.POINTER(gpis_cam)]
    L.gpis3_update.argtypes = [vp, fp, C.c_int, fp]
    L.gpis3_test.argtypes = [vp, fp, C.c_int, C.c_int, fp]
    L.gpis3_test_device.argtypes = [vp, vp, C.c_int, vp, vp]
    L.gpis3_num_points.argtypes = [vp]
    L.gpis3_save.argtypes = [vp, C.c_char_p]
    L.gpis3_load.argtypes = [vp, C.c_char_p]
    L.gpis3_get_points.argtypes = [vp, fp, C.c_int]
    L.gpis3_get_nodes.argtypes = [vp, fp, C.c_int]
    L.gpis3_stats.argtypes = [vp, dp, C.c_int]
    L.gpis3_pass_jobs.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.gpis3_set_profile.argtypes = [vp, C.c_int]
    L.gpis3_sync.argtypes = [vp]
    L.gpis3_set_pipeline.argtypes = [vp, C.c_int]
    L.gpis3_set_host_gather.argtypes = [vp, C.c_int]
    L.gpis3_set_keep_factors.argtypes = [vp, C.c_int]
    L.gpis3_set_shard_factors.argtypes = [vp, C.c_int]
    L.gpis2_create.restype = vp
    L.gpis2_destroy.argtypes = [vp]
    L.gpis2_reset.argtypes = [vp]
    L.gpis2_update.argtypes = [vp, fp, fp, C.c_int, fp]
    L.gpis2_test.argtypes = [vp, fp, C.c_int, C.c_int, fp]
    L.gpis2_test_device.argtypes = [vp, vp, C.c_int, vp, vp]
    L.gpis2_get_nodes.argtypes = [vp, fp, C.c_int]
    L.gpis2_stats.argtypes = [vp, dp, C.c_int]
    L.gpis2_pass_jobs.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(L, "gpis3_set_pass2_mode"):
        for name in ("gpis3", "gpis2", "gpis_mapquery"):
            getattr(L, name + "_set_pass2_mode").argtypes = [vp, C.c_int]
            getattr(L, name + "_pass_detail").argtypes = [vp, dp]
    if hasattr(L, "gpis3_set_k4_schedule"):
        L.gpis3_set_k4_schedule.argtypes = [vp, C.c_int]
        L.gpis_mapquery_set_k4_schedule.argtypes = [vp, C.c_int]
        L.gpis_mapquery_last_counts.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(L, "gpis2_sync"):
        L.gpis2_sync.argtypes = [vp]
        L.gpis2_set_pipeline.argtypes = [vp, C.c_int]
    L.gpis_obsgp_create.restype = vp
    L.gpis_obsgp_destroy.argtypes = [vp]
    L.gpis_obsgp_train2d.argtypes = [vp, fp, fp, C.c_int, C.c_int]
    L.gpis_obsgp_train1d.argtypes = [vp, fp, fp, C.c_int]
    L.gpis_obsgp_query.argtypes = [vp, fp, C.c_int, fp, fp]
    L.gpis_obsgp_query_route.argtypes = [vp, C.c_int, fp, C.c_int, fp, fp]
    L.gpis_obsgp_pending.argtypes = [vp]
    L.gpis_obsgp_num_groups.argtypes = [vp]
    L.gpis_obsgp_get_group.argtypes = [vp, C.c_int, ip, fp, fp, fp]
    L.gpis_ongpis_create.restype = vp
    L.gpis_ongpis_create.argtypes = [C.c_int, C.c_float]
    L.gpis_ongpis_destroy.argtypes = [vp]
    L.gpis3_create_multi.restype = vp
    L.gpis3_create_multi.argtypes = [C.c_void_p, ip, C.c_int]
    L.gpis3_num_devices.argtypes = [vp]
    L.gpis_ongpis_train.argtypes = [vp, fp, C.c_int, ip, ip, C.c_int, ip]
    L.gpis_ongpis_model_dims.argtypes = [vp, C.c_int, ip]
    L.gpis_ongpis_get_model.argtypes = [vp, C.c_int, fp, fp, ip]
    L.gpis_ongpis_eval.argtypes = [vp, fp, C.c_int, ip, ip, C.c_int, fp]
    L.gpis_ongpis_eval_layout.argtypes = [vp, fp, C.c_int, ip, ip, C.c_int, C.c_int, fp]
    L.gpis_ongpis_last_ms.argtypes = [vp, fp, fp]
    L.gpis_ongpis_set_exp_table.argtypes = [vp, C.c_int]
    L.gpis_ongpis_kernel_matrix.argtypes = [vp, fp, ip, fp, fp, C.c_int, fp]
    L.gpis_ongpis_set_debug.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "gpis_ongpis_set_cu_reserve"):
        L.gpis_ongpis_set_cu_reserve.argtypes = [vp, C.c_int]
    if hasattr(L, "gpis_selftest_ranged_arith"):       # (A/B runs load older builds of the library through GPISMAP_AMD_LIB)
        L.gpis_selftest_ranged_arith.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        L.gpis_selftest_ranged_arith.restype = C.c_int
    L.gpis_ongpis_set_keep_factor.argtypes = [vp, C.c_int]
    L.gpis_ongpis_set_fused.argtypes = [vp, C.c_int]
    L.gpis_ongpis_set_lazy_inverse.argtypes = [vp, C.c_int]
    L.gpis3_prepare_test.argtypes = [vp]
    L.gpis3_set_lazy_inverse.argtypes = [vp, C.c_int]
    if hasattr(L, "gpis_mapquery_create"):
        L.gpis_mapquery_create.restype = vp
        L.gpis_mapquery_create.argtypes = [vp, C.c_float, C.c_float, C.c_float]
        L.gpis_mapquery_destroy.argtypes = [vp]
        L.gpis_mapquery_set_table.argtypes = [vp, C.c_int, fp, fp, fp, ip, ip, C.c_int, fp, fp, ip, C.c_double]
        L.gpis_mapquery_set_chunk.argtypes = [vp, C.c_int]
        L.gpis_mapquery_run.argtypes = [vp, fp, C.c_int, fp]
        if hasattr(L, "gpis_mapquery_run_device"):
            L.gpis_mapquery_run_device.argtypes = [vp, vp, C.c_int, vp, vp]
        L.gpis_mapquery_candidates.argtypes = [vp, ip, ip]
        L.gpis_mapquery_pass_jobs.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(L, "gpis_mesh_create"):
        L.gpis_mesh_create.restype = vp
        L.gpis_mesh_create.argtypes = []
        L.gpis_mesh_destroy.argtypes = [vp]
        L.gpis_mesh_set_chunk.argtypes = [vp, C.c_int]
        L.gpis_mesh_from_grid.argtypes = [vp, vp, C.c_int, ip, fp, fp, C.c_float, vp]
        L.gpis3_extract_mesh.argtypes = [vp, vp, ip, fp, fp, C.c_float, vp]
        L.gpis2_extract_contour.argtypes = [vp, vp, ip, fp, fp, C.c_float, vp]
        L.gpis_mesh_counts.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.gpis_mesh_get.argtypes = [vp, fp, ip, fp]
        L.gpis_mesh_get_grid.argtypes = [vp, fp]
        L.gpis_mesh_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    if hasattr(L, "gpis_dfield_create"):
        L.gpis_dfield_create.restype = vp
        L.gpis_dfield_create.argtypes = []
        L.gpis_dfield_destroy.argtypes = [vp]
        L.gpis_dfield_set_chunk.argtypes = [vp, C.c_int]
        L.gpis_dfield_from_grid.argtypes = [vp, vp, C.c_int, ip, fp, fp, C.c_float, vp]
        L.gpis3_distance_field.argtypes = [vp, vp, ip, fp, fp, C.c_float, C.c_float, vp]
        L.gpis2_distance_field.argtypes = [vp, vp, ip, fp, fp, C.c_float, C.c_float, vp]
        L.gpis_dfield_info.argtypes = [vp, ip, ip, fp, fp]
        L.gpis_dfield_get.argtypes = [vp, fp, ip, fp]
        L.gpis_dfield_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.gpis_dfield_sample.argtypes = [vp, vp, C.c_longlong, vp, vp]
    if hasattr(L, "gpis_render_create"):
        L.gpis_render_default_opts.argtypes = [C.c_int, C.POINTER(gpis_render_opts)]
        L.gpis_render_create.restype = vp
        L.gpis_render_create.argtypes = []
        L.gpis_render_destroy.argtypes = [vp]
        L.gpis_render_set_chunk.argtypes = [vp, C.c_int]
        L.gpis3_render_depth.argtypes = [vp, vp, C.POINTER(gpis_cam), fp, C.POINTER(gpis_render_opts), vp]
        L.gpis2_render_scan.argtypes = [vp, vp, fp, C.c_int, fp, C.POINTER(gpis_render_opts), vp]
        L.gpis_render_get.argtypes = [vp, fp, fp, C.POINTER(C.c_ubyte)]
        L.gpis_render_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.gpis_render_info.argtypes = [vp, dp, C.c_int]
    if hasattr(L, "gpis_track_create"):
        L.gpis_track_default_opts.argtypes = [C.c_int, C.POINTER(gpis_track_opts)]
        L.gpis_track_create.restype = vp
        L.gpis_track_create.argtypes = []
        L.gpis_track_destroy.argtypes = [vp]
        L.gpis_track_set_chunk.argtypes = [vp, C.c_int]
        L.gpis3_track_depth.argtypes = [vp, vp, C.POINTER(gpis_cam), fp, fp, C.POINTER(gpis_track_opts), fp, vp]
        L.gpis2_track_scan.argtypes = [vp, vp, fp, fp, C.c_int, fp, C.POINTER(gpis_track_opts), fp, vp]
        L.gpis_track_get.argtypes = [vp, dp, dp, fp]
        L.gpis_track_info.argtypes = [vp, dp, C.c_int]
    if hasattr(L, "gpis3_track_depth_field"):
        L.gpis3_track_depth_field.argtypes = [vp, vp, vp, C.POINTER(gpis_cam), fp, fp, C.POINTER(gpis_track_opts), fp, vp]
        L.gpis2_track_scan_field.argtypes = [vp, vp, vp, fp, fp, C.c_int, fp, fp, C.POINTER(gpis_track_opts), fp, vp]
    if hasattr(L, "gpis3_render_depth_field"):
        fo = C.POINTER(gpis_render_field_opts)
        L.gpis_render_field_default_opts.argtypes = [C.c_int, C.c_float, fo]
        L.gpis_render_set_field_tiles.argtypes = [vp, C.c_int]
        L.gpis3_render_depth_field.argtypes = [vp, vp, vp, C.POINTER(gpis_cam), fp, fo, vp]
        L.gpis2_render_scan_field.argtypes = [vp, vp, vp, fp, C.c_int, fp, fp, fo, vp]
    if hasattr(L, "gpis_plan_create"):
        ll, ub = C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)
        L.gpis_plan_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpis_plan_opts)]
        L.gpis_plan_create.restype = vp
        L.gpis_plan_create.argtypes = []
        L.gpis_plan_destroy.argtypes = [vp]
        L.gpis_plan_solve.argtypes = [vp, vp, fp, C.c_int, C.POINTER(gpis_plan_opts), vp]
        L.gpis_plan_info.argtypes = [vp, dp, C.c_int]
        L.gpis_plan_get.argtypes = [vp, fp, ub]
        L.gpis_plan_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.gpis_plan_paths.argtypes = [vp, fp, C.c_int, C.c_int, vp]
        L.gpis_plan_path_counts.argtypes = [vp, ll, ll]
        L.gpis_plan_get_paths.argtypes = [vp, ll, fp, fp, ub]
        L.gpis_plan_set_schedule.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "gpis_pplan_create"):
        ll, ub = C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)
        L.gpis_pplan_default_opts.argtypes = [C.c_float, C.c_int, C.POINTER(gpis_pplan_opts)]
        L.gpis_pplan_create.restype = vp
        L.gpis_pplan_create.argtypes = []
        L.gpis_pplan_destroy.argtypes = [vp]
        L.gpis_pplan_solve.argtypes = [vp, vp, vp, dp, C.POINTER(C.c_ushort), C.c_int, fp, C.c_int, C.POINTER(gpis_pplan_opts), vp]
        L.gpis_pplan_info.argtypes = [vp, dp, C.c_int]
        L.gpis_pplan_get.argtypes = [vp, fp, ub, fp]
        L.gpis_pplan_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.gpis_pplan_paths.argtypes = [vp, fp, C.c_int, C.c_int, vp]
        L.gpis_pplan_path_counts.argtypes = [vp, ll, ll]
        L.gpis_pplan_get_paths.argtypes = [vp, ll, fp, ip, fp, ub]
        L.gpis_pplan_project.argtypes = [vp, vp, ub]
        L.gpis_pplan_set_schedule.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "gpis_traj_create"):
        ub = C.POINTER(C.c_ubyte)
        L.gpis_traj_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpis_traj_opts)]
        L.gpis_traj_create.restype = vp
        L.gpis_traj_create.argtypes = []
        L.gpis_traj_destroy.argtypes = [vp]
        L.gpis_traj_from_paths.argtypes = [vp, vp, C.c_int]
        L.gpis_traj_set.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int]
        L.gpis_traj_optimize.argtypes = [vp, vp, C.POINTER(gpis_traj_opts), vp]
        L.gpis_traj_info.argtypes = [vp, dp, C.c_int]
        L.gpis_traj_get.argtypes = [vp, fp, ub, ip, fp, fp, fp, fp, ip, ub]
        L.gpis_traj_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    if hasattr(L, "gpis_timing_time"):
        ub = C.POINTER(C.c_ubyte)
        d = C.c_double
        L.gpis_timing_default_opts.argtypes = [C.c_int, C.c_float, C.POINTER(gpis_traj_timing_opts)]
        L.gpis_timing_time.argtypes = [vp, vp, C.POINTER(gpis_traj_timing_opts), vp]
        L.gpis_timing_info.argtypes = [vp, dp, C.c_int]
        L.gpis_timing_get.argtypes = [vp, fp, fp, ub, ub, fp, fp, fp, ip]
        L.gpis_timing_controls.argtypes = [vp, d, C.c_int, d, d, d, dp, dp, dp, ip]
        L.gpis_timing_follow.argtypes = [vp, vp, C.c_int, d, d, d, d, dp, dp]
    if hasattr(L, "gpis_locate_create"):
        lo = C.POINTER(gpis_locate_opts)
        L.gpis_locate_default_opts.argtypes = [C.c_int, lo]
        L.gpis_locate_create.restype = vp
        L.gpis_locate_create.argtypes = []
        L.gpis_locate_destroy.argtypes = [vp]
        L.gpis3_locate_depth_field.argtypes = [vp, vp, vp, C.POINTER(gpis_cam), fp, fp, C.c_int, lo, vp]
        L.gpis2_locate_scan_field.argtypes = [vp, vp, vp, fp, fp, C.c_int, fp, fp, C.c_int, lo, vp]
        L.gpis_locate_get.argtypes = [vp, dp, ip, ip]
        L.gpis_locate_info.argtypes = [vp, dp, C.c_int]
        L.gpis_locate_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    if hasattr(L, "gpis_pf_create"):
        po = C.POINTER(gpis_pf_opts)
        u64p = C.POINTER(C.c_ulonglong)
        L.gpis_pf_default_opts.argtypes = [C.c_int, po]
        L.gpis_pf_create.restype = vp
        L.gpis_pf_create.argtypes = []
        L.gpis_pf_destroy.argtypes = [vp]
        L.gpis_pf_init.argtypes = [vp, C.c_int, fp, C.c_int, C.c_ulonglong]
        L.gpis_pf_predict.argtypes = [vp, dp, po, vp]
        L.gpis2_pf_update_scan.argtypes = [vp, vp, vp, fp, fp, C.c_int, fp, po, vp]
        L.gpis3_pf_update_depth.argtypes = [vp, vp, vp, C.POINTER(gpis_cam), fp, po, vp]
        L.gpis_pf_resample.argtypes = [vp, vp]
        L.gpis_pf_estimate.argtypes = [vp, dp, dp, u64p, ip]
        L.gpis_pf_get.argtypes = [vp, dp, dp, u64p, dp, ip, ip, fp]
        L.gpis_pf_device.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int]
        L.gpis_pf_info.argtypes = [vp, dp, C.c_int]
    if hasattr(L, "gpis_mppi_create"):
        mo = C.POINTER(gpis_mppi_opts)
        L.gpis_mppi_default_opts.argtypes = [C.c_int, C.c_float, mo]
        L.gpis_mppi_create.restype = vp
        L.gpis_mppi_create.argtypes = []
        L.gpis_mppi_destroy.argtypes = [vp]
        L.gpis_mppi_init.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_ulonglong]
        L.gpis_mppi_set_nominal.argtypes = [vp, dp]
        L.gpis_mppi_step.argtypes = [vp, vp, vp, dp, dp, mo, dp, vp]
        L.gpis_mppi_shift.argtypes = [vp]
        L.gpis_mppi_get.argtypes = [vp, dp, dp, C.POINTER(C.c_ulonglong), ip, dp, dp]
        L.gpis_mppi_device.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int]
        L.gpis_mppi_info.argtypes = [vp, dp, C.c_int]
    if hasattr(L, "gpis_obst_create"):
        oo = C.POINTER(gpis_obst_opts)
        L.gpis_obst_default_opts.argtypes = [C.c_int, C.c_float, oo]
        L.gpis_obst_create.restype = vp
        L.gpis_obst_create.argtypes = []
        L.gpis_obst_destroy.argtypes = [vp]
        L.gpis_obst_set.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, d]
        L.gpis_obst_set_opts.argtypes = [vp, oo]
        L.gpis_obst_get.argtypes = [vp, dp, dp, dp, oo]
        L.gpis_obst_info.argtypes = [vp, dp, C.c_int]
        L.gpis_obst_at.argtypes = [vp, d, dp]
        L.gpis_obst_mppi_step.argtypes = [vp, vp, vp, vp, d, dp, dp, C.POINTER(gpis_mppi_opts), dp, vp]
        L.gpis_obst_mppi_get.argtypes = [vp, ip, dp, dp]
        L.gpis_obst_check_timing.argtypes = [vp, vp, d, C.c_int, d, d, d, dp, dp, ip, ip, ip]
    if hasattr(L, "gpis_retime_solve"):
        ro = C.POINTER(gpis_retime_opts)
        L.gpis_retime_default_opts.argtypes = [C.c_int, C.c_float, ro]
        L.gpis_retime_solve.argtypes = [vp, vp, d, ro, vp]
        L.gpis_retime_get.argtypes = [vp, ip, ip, ip, ip, ip, ip, ro, dp]
        L.gpis_retime_controls.argtypes = [vp, C.c_int, C.c_int, d, d, dp, dp, dp, ip]
        L.gpis_retime_follow.argtypes = [vp, vp, C.c_int, C.c_int, d, d, dp, dp]
        L.gpis_retime_check.argtypes = [vp, vp, C.c_int, d, dp, dp, ip, ip, ip]
    if hasattr(L, "gpis_tplan_create"):
        to, ub, ll = C.POINTER(gpis_tplan_opts), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong)
        L.gpis_tplan_default_opts.argtypes = [C.c_float, to]
        L.gpis_tplan_check_opts.argtypes = [to, C.c_int, C.c_int]
        L.gpis_tplan_create.restype = vp
        L.gpis_tplan_create.argtypes = []
        L.gpis_tplan_destroy.argtypes = [vp]
        L.gpis_tplan_solve.argtypes = [vp, vp, vp, fp, C.c_int, d, to, vp]
        L.gpis_tplan_info.argtypes = [vp, dp, C.c_int]
        L.gpis_tplan_get.argtypes = [vp, fp, ub, fp, fp]
        L.gpis_tplan_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.gpis_tplan_paths.argtypes = [vp, fp, C.c_int, vp]
        L.gpis_tplan_path_counts.argtypes = [vp, ll, ll]
        L.gpis_tplan_get_paths.argtypes = [vp, ll, fp, ip, fp, ub]
        L.gpis_tplan_check.argtypes = [vp, vp, d, dp, dp, ip, ip, ip]
        L.gpis_tplan_controls.argtypes = [vp, C.c_int, C.c_int, d, d, dp, dp, dp, ip]
        L.gpis_tplan_set_schedule.argtypes = [vp, C.c_int, C.c_int]
    if hasattr(L, "gpis_tpplan_create"):
        to, ub, ll, us = C.POINTER(gpis_tpplan_opts), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong), C.POINTER(C.c_ushort)
        L.gpis_tpplan_default_opts.argtypes = [C.c_float, C.c_int, to]
        L.gpis_tpplan_check_opts.argtypes = [to, C.c_int, C.c_int, C.c_int]
        L.gpis_tpplan_create.restype = vp
        L.gpis_tpplan_create.argtypes = []
        L.gpis_tpplan_destroy.argtypes = [vp]
        L.gpis_tpplan_solve.argtypes = [vp, vp, vp, vp, dp, us, C.c_int, fp, C.c_int, d, to, vp]
        L.gpis_tpplan_info.argtypes = [vp, dp, C.c_int]
        L.gpis_tpplan_get.argtypes = [vp, fp, ub, fp, fp]
        L.gpis_tpplan_paths.argtypes = [vp, fp, C.c_int, vp]
        L.gpis_tpplan_path_counts.argtypes = [vp, ll, ll]
        L.gpis_tpplan_get_paths.argtypes = [vp, ll, fp, ip, ip, fp, ub]
        L.gpis_tpplan_check.argtypes = [vp, vp, vp, d, dp, dp, ip, ip, ip, ip]
        L.gpis_tpplan_controls.argtypes = [vp, C.c_int, C.c_int, d, d, dp, dp, dp, ip]
        L.gpis_tpplan_set_schedule.argtypes = [vp, C.c_int]
    if hasattr(L, "gpis_body_create"):
        L.gpis_body_create.restype = vp
        L.gpis_body_create.argtypes = []
        L.gpis_body_destroy.argtypes = [vp]
        L.gpis_body_set.argtypes = [vp, C.c_int, C.c_int, dp, dp]
        L.gpis_body_get.argtypes = [vp, dp, dp]
        L.gpis_body_info.argtypes = [vp, dp, C.c_int]
        L.gpis_body_clearance.argtypes = [vp, vp, dp, C.c_longlong, d, dp, ip, ip, vp]
        L.gpis_body_mppi_step.argtypes = [vp, vp, vp, vp, vp, d, dp, dp, C.POINTER(gpis_mppi_opts), dp, vp]
        L.gpis_body_traj_clearance.argtypes = [vp, vp, vp, d, dp, ip, ip, ip]
    if hasattr(L, "gpis_timed_body_check"):
        L.gpis_timed_body_check.argtypes = [vp, vp, vp, d, C.c_int, d, d, d, dp, dp, ip, ip, ip, ip]
        L.gpis_timed_body_retime.argtypes = [vp, vp, vp, d, C.POINTER(gpis_retime_opts), vp]
        L.gpis_timed_body_info.argtypes = [vp, dp, C.c_int]
        L.gpis_timed_body_retime_check.argtypes = [vp, vp, vp, C.c_int, d, dp, dp, ip, ip, ip, ip]
        L.gpis_timed_body_states.argtypes = [vp, d, C.c_int, d, C.c_int, dp]
    if hasattr(L, "gpis_smooth_body_optimize"):
        L.gpis_smooth_body_default_opts.argtypes = [C.c_int, C.c_float, C.c_int, C.POINTER(gpis_traj_opts), C.POINTER(C.c_float)]
        L.gpis_smooth_body_optimize.argtypes = [vp, vp, vp, C.POINTER(gpis_traj_opts), C.c_float, vp]
        L.gpis_smooth_body_get.argtypes = [vp, dp, ip, ip, ip]
        L.gpis_smooth_from_pose_paths.argtypes = [vp, vp, C.c_int]
    if hasattr(L, "gpis_cover_create"):
        co, ub, ll = C.POINTER(gpis_cover_opts), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong)
        L.gpis_cover_default_opts.argtypes = [C.c_int, C.c_float, co]
        L.gpis_cover_create.restype = vp
        L.gpis_cover_create.argtypes = []
        L.gpis_cover_destroy.argtypes = [vp]
        L.gpis_cover_reset.argtypes = [vp, vp]
        L.gpis_cover_set.argtypes = [vp, ub, C.c_longlong]
        L.gpis_cover_get.argtypes = [vp, ub, C.c_longlong]
        L.gpis_cover_device.argtypes = [vp, C.POINTER(C.c_void_p)]
        L.gpis3_cover_depth.argtypes = [vp, vp, C.POINTER(gpis_cam), fp, fp, co, vp]
        L.gpis2_cover_scan.argtypes = [vp, vp, fp, fp, C.c_int, fp, fp, co, vp]
        L.gpis_cover_frontiers.argtypes = [vp, vp, co, vp]
        L.gpis_cover_counts.argtypes = [vp, ll, ll, ll]
        L.gpis_cover_get_frontiers.argtypes = [vp, ip, ip, ll, ip, ip, ip, ip]
        L.gpis_cover_restrict.argtypes = [vp, vp, vp, C.c_float, vp]
        L.gpis_cover_info.argtypes = [vp, dp, C.c_int]
    if hasattr(L, "gpis_view_create"):
        vo = C.POINTER(gpis_view_opts)
        L.gpis_view_default_opts.argtypes = [C.c_int, C.c_float, vo]
        L.gpis_view_create.restype = vp
        L.gpis_view_create.argtypes = []
        L.gpis_view_destroy.argtypes = [vp]
        L.gpis3_view_gain_depth.argtypes = [vp, vp, vp, vp, C.POINTER(gpis_cam), fp, C.c_int, vo, vp]
        L.gpis2_view_gain_scan.argtypes = [vp, vp, vp, vp, fp, C.c_int, fp, fp, C.c_int, vo, vp]
        L.gpis_view_get.argtypes = [vp, C.POINTER(C.c_longlong), ip, C.c_int]
        L.gpis_view_get_predicted.argtypes = [vp, C.c_int, fp, C.c_longlong]
        L.gpis_view_info.argtypes = [vp, dp, C.c_int]
    if hasattr(L, "gpis_detect_create"):
        do, ub, ll = C.POINTER(gpis_detect_opts), C.POINTER(C.c_ubyte), C.POINTER(C.c_longlong)
        L.gpis_detect_default_opts.argtypes = [C.c_int, C.c_float, do]
        L.gpis_detect_create.restype = vp
        L.gpis_detect_create.argtypes = []
        L.gpis_detect_destroy.argtypes = [vp]
        L.gpis_detect_set_schedule.argtypes = [vp, C.c_int, C.c_int]
        L.gpis_detect_reset_tracks.argtypes = [vp]
        L.gpis3_detect_depth_field.argtypes = [vp, vp, vp, vp, C.POINTER(gpis_cam), fp, dp, C.c_double, do, vp]
        L.gpis2_detect_scan_field.argtypes = [vp, vp, vp, vp, fp, fp, C.c_int, fp, dp, C.c_double, do, vp]
        L.gpis_detect_counts.argtypes = [vp, ll, ll, ll]
        L.gpis_detect_get_balls.argtypes = [vp, dp, dp, dp, ip, fp, ip, ip, ip, ip]
        L.gpis_detect_get_components.argtypes = [vp, ip, ip, fp, dp, dp, ip]
        L.gpis_detect_get_samples.argtypes = [vp, ip, fp, fp, ub]
        L.gpis_detect_to_obstacles.argtypes = [vp, vp]
        L.gpis_detect_info.argtypes = [vp, dp, C.c_int]
    _lib = L
    return L


def selftest_ranged_arith(seed=1, blocks=1024, per_thread=64, mode=0):
    """gpis_selftest_ranged_arith: (square-root mismatches, division mismatches) of blocks * 256 * per_thread operand pairs run
    through the factorisation kernels' range-restricted sqrt / division and through the compiler's IEEE ones on the device."""
    m = (C.c_ulonglong * 2)(0, 0)
    _check(lib().gpis_selftest_ranged_arith(int(seed), int(blocks), int(per_thread), int(mode), m), "gpis_selftest_ranged_arith")
    return int(m[0]), int(m[1])


def pool_cache_trim():
    """Hand the device-pool chunks the library caches across maps back to the driver (gpis_pool_cache_trim); bytes released."""
    return int(lib().gpis_pool_cache_trim()) if (_lib is not None or os.path.exists(LIB_PATH)) else 0


def _trim_at_exit():
    # only if the library was ever loaded: the cache holds memory of DESTROYED pools, nothing a live map uses
    if _lib is not None:
        try:
            _lib.gpis_pool_cache_trim()
        except Exception:
            pass


import atexit as _atexit  # noqa: E402
_atexit.register(_trim_at_exit)


def device_count():
    return lib().gpis_device_count()


def set_device(device):
    """Select the HIP device for every object created afterwards (one process per GPU: LOCAL_RANK)."""
    _check(lib().gpis_set_device(int(device)), "gpis_set_device(%d)" % int(device))


def get_device():
    return lib().gpis_get_device()


def _check(rc, what):
    if rc != 0:
        raise GpisError("%s failed with status %d" % (what, rc))


def _cam(cam6):
    c = np.asarray(cam6, dtype=np.float64)
    return gpis_cam(float(c[0]), float(c[1]), float(c[2]), float(c[3]), int(c[4]), int(c[5]))


def _depth_frame(what, depth, cam6, map_h, map_wh):
    """A depth frame for the C-ABI: (depth [W*H] f32, or None for a call that takes no image; the gpis_cam argument).  cam6
    None = the camera of the map `map_h`, whose (width, height) is map_wh."""
    if cam6 is None and map_h is None:
        raise GpisError("a field-only %s needs cam6" % what)
    if depth is not None:
        depth = np.ascontiguousarray(depth, dtype=np.float32).ravel()
        w, h = (int(cam6[4]), int(cam6[5])) if cam6 is not None else map_wh
        if depth.size != w * h:
            raise GpisError("depth must have width * height = %d elements" % (w * h))
    return depth, (C.byref(_cam(cam6)) if cam6 is not None else None)


def _scan_frame(what, thetas, ranges, off2, map_h):
    """A scan frame for the C-ABI: (thetas [n] f32, ranges [n] f32 or None for a call that takes none, the off2 argument).  off2
    None = the sensor offset of the map `map_h`."""
    thetas = np.ascontiguousarray(thetas, dtype=np.float32).ravel()
    if ranges is not None:
        ranges = np.ascontiguousarray(ranges, dtype=np.float32).ravel()
        if thetas.size != ranges.size:
            raise GpisError("thetas and ranges differ in size")
    if off2 is None:
        if map_h is None:
            raise GpisError("a field-only %s needs off2" % what)
        return thetas, ranges, None
    off = np.ascontiguousarray(off2, dtype=np.float32).ravel()
    if off.size != 2:
        raise GpisError("off2 must have 2 elements")
    return thetas, ranges, _p(off)


class GPisMap3:
    """Mirror of the reference's mexGPisMap3 command set on the HIP path."""

    STAT_KEYS = ("obsgp_groups", "obsgp_queries", "clusters_trained", "late_reevals", "clusters",
                 "last_test_evals", "last_test_k4_ms", "device_bytes", "last_test_flops", "last_test_k4_launches",
                 "last_train_ms", "model_bytes", "upd_preproc_ms", "upd_obsgp_train_ms", "upd_reeval_ms", "upd_eval_ms",
                 "upd_gps_ms", "last_train_flops", "last_train_bytes", "last_train_jobs", "last_train_maxK",
                 "last_inverse_ms", "last_inverse_jobs", "exchange_bytes", "pipelined", "train_cu_reserve", "host_replays", "deferred_inverses")

    def __init__(self, cam6=None, devices=None):
        """devices: list of HIP device ids for ONE map over several devices (gpis3_create_multi; a device may repeat:
        logical shards on one GPU); None = the current device (or GPIS_DEVICES from the environment)."""
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        cam = C.byref(_cam(cam6)) if cam6 is not None else None
        self._wh = (640, 480) if cam6 is None else (int(cam6[4]), int(cam6[5]))    # (the reference's default camera)
        if devices is None:
            self.h = C.c_void_p(self.L.gpis3_create(cam))
        else:
            d = np.ascontiguousarray(devices, dtype=np.int32)
            self.h = C.c_void_p(self.L.gpis3_create_multi(cam, _p(d, C.c_int), d.size))
        if not self.h:
            raise GpisError("gpis3_create failed")

    def num_devices(self):
        return int(self.L.gpis3_num_devices(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis3_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _check(self.L.gpis3_reset(self.h), "gpis3_reset")

    def set_camera(self, cam6):
        _check(self.L.gpis3_set_camera(self.h, C.byref(_cam(cam6))), "gpis3_set_camera")
        self._wh = (int(cam6[4]), int(cam6[5]))

    def update(self, depth, pose):
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        pose = np.ascontiguousarray(pose, dtype=np.float32)
        if pose.size != 12:
            raise GpisError("pose must have 12 elements")
        _check(self.L.gpis3_update(self.h, _p(depth), depth.size, _p(pose)), "gpis3_update")

    def test(self, x, res=None):
        """x: [N,3] float32.  Returns res [N,8] (zero pre-filled like the mex gateway) or None
        where the reference's test() returns false."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if res is None:
            res = np.zeros((x.shape[0], 8), dtype=np.float32)
        rc = self.L.gpis3_test(self.h, _p(x), 3, x.shape[0], _p(res))
        if rc == -1:
            return None
        _check(rc, "gpis3_test")
        return res

    def test_device(self, d_x_ptr, n, d_res_ptr, stream=0):
        _check(self.L.gpis3_test_device(self.h, C.c_void_p(d_x_ptr), n, C.c_void_p(d_res_ptr), C.c_void_p(stream)),
               "gpis3_test_device")

    def device(self):
        return self.L.gpis3_device(self.h)

    # ---- sharded training (include/gpismap_amd.h, gpis3_set_shard ...) ----
    def set_shard(self, rank, world):
        _check(self.L.gpis3_set_shard(self.h, int(rank), int(world)), "gpis3_set_shard")
        self._world = int(world)

    def shard_info(self):
        w = getattr(self, "_world", 1)
        out = np.zeros(2 + w, dtype=np.int32)
        _check(self.L.gpis3_shard_info(self.h, _p(out, C.c_int), 2 + w), "gpis3_shard_info")
        return int(out[0]), int(out[1]), [int(v) for v in out[2:]]

    def shard_bytes(self, owner):
        """Bytes of rank `owner`'s packed records of the last update (records back to back at their own sizes; every rank
        gives the same answer for every owner)."""
        b = int(self.L.gpis3_shard_bytes(self.h, int(owner)))
        if b < 0:
            raise GpisError("gpis3_shard_bytes failed (%d)" % b)
        return b

    def shard_pack(self, d_buf_ptr, stream=0):
        _check(self.L.gpis3_shard_pack(self.h, C.c_void_p(d_buf_ptr), C.c_void_p(stream)), "gpis3_shard_pack")

    def shard_unpack(self, owner, d_buf_ptr, stream=0):
        _check(self.L.gpis3_shard_unpack(self.h, int(owner), C.c_void_p(d_buf_ptr), C.c_void_p(stream)), "gpis3_shard_unpack")

    def shard_finish(self):
        _check(self.L.gpis3_shard_finish(self.h), "gpis3_shard_finish")

    # ---- one process per GPU, host logic once (gpis3_set_frame_export ...; gpismap_amd.sharding.update_lead_worker) ----
    def set_frame_export(self, on=True):
        _check(self.L.gpis3_set_frame_export(self.h, 1 if on else 0), "gpis3_set_frame_export")

    def frame_record(self):
        """The record of the last update() on the lead (numpy uint8)."""
        n = int(self.L.gpis3_frame_record(self.h, None, 0))
        if n < 0:
            raise GpisError("gpis3_frame_record failed (%d)" % n)
        buf = np.empty(max(n, 1), dtype=np.uint8)
        m = int(self.L.gpis3_frame_record(self.h, buf.ctypes.data_as(C.c_void_p), n))
        if m != n:
            raise GpisError("gpis3_frame_record failed (%d)" % m)
        return buf[:n]

    def train_deferred(self):
        _check(self.L.gpis3_train_deferred(self.h), "gpis3_train_deferred")

    def apply_frame(self, record):
        record = np.ascontiguousarray(record, dtype=np.uint8)
        _check(self.L.gpis3_apply_frame(self.h, record.ctypes.data_as(C.c_void_p), int(record.size)), "gpis3_apply_frame")

    def num_points(self):
        return self.L.gpis3_num_points(self.h)

    def get_all_points(self):
        n = self.L.gpis3_get_points(self.h, None, 0)
        out = np.zeros((n, 3), dtype=np.float32)
        if n:
            self.L.gpis3_get_points(self.h, _p(out), n)
        return out

    def nodes(self):
        n = self.L.gpis3_get_nodes(self.h, None, 0)
        out = np.zeros((n, 9), dtype=np.float32)
        if n:
            self.L.gpis3_get_nodes(self.h, _p(out), n)
        return out

    def stats(self):
        a = (C.c_double * 28)()
        _check(self.L.gpis3_stats(self.h, a, 28), "gpis3_stats")
        return dict(zip(self.STAT_KEYS, list(a)))

    PASS_KEYS = ("pass1", "pass2_full", "pass2a_value", "pass2b_grad")

    def pass_jobs(self):
        """K4 jobs of the last test() per evaluation pass (gpis3_pass_jobs)."""
        a = (C.c_longlong * 4)()
        _check(self.L.gpis3_pass_jobs(self.h, a), "gpis3_pass_jobs")
        return dict(zip(self.PASS_KEYS, list(a)))

    DETAIL_KEYS = ("predicted_full", "value_only", "repair", "unread", "predictions", "hits", "pick_ms", "mode")

    def set_pass2_mode(self, mode):
        """How test() evaluates candidates 2 and 3 of a three-candidate fallback: 0 value columns first, 1 the predicted candidate
        in full (default), 2 / 3 always candidate 2 / 3, 4 the predictor inverted.  Same results in every mode (gpis3_set_pass2_mode)."""
        _check(self.L.gpis3_set_pass2_mode(self.h, int(mode)), "gpis3_set_pass2_mode")

    def set_k4_schedule(self, mode):
        """How test() cuts a call into chunks: 0 chunks of 2^22 queries, 1 (default) the whole call in one chunk where the device
        has the memory.  Same results (gpis3_set_k4_schedule)."""
        _check(self.L.gpis3_set_k4_schedule(self.h, int(mode)), "gpis3_set_k4_schedule")

    def pass_detail(self):
        """How the prediction of the last test() went (gpis3_pass_detail)."""
        a = (C.c_double * 8)()
        _check(self.L.gpis3_pass_detail(self.h, a), "gpis3_pass_detail")
        return dict(zip(self.DETAIL_KEYS, list(a)))

    def save(self, path):
        """Map checkpoint: spatial index, surface points and the packed prediction records of the trained models (gpis3_save)."""
        _check(self.L.gpis3_save(self.h, os.fsencode(path)), "gpis3_save")

    def load(self, path):
        """Replace the map's state with a checkpoint's; models are restored verbatim, nothing is retrained (gpis3_load)."""
        _check(self.L.gpis3_load(self.h, os.fsencode(path)), "gpis3_load")

    def set_profile(self, on=True):
        _check(self.L.gpis3_set_profile(self.h, int(on)), "gpis3_set_profile")

    def prepare_test(self):
        """Join a pipelined training and compute the inverses the last updates left to the first test()."""
        _check(self.L.gpis3_prepare_test(self.h), "gpis3_prepare_test")

    def set_lazy_inverse(self, on=True):
        _check(self.L.gpis3_set_lazy_inverse(self.h, int(on)), "gpis3_set_lazy_inverse")

    def sync(self):
        """Join the training the last update() left in flight (pipelined update, include/gpismap_amd.h)."""
        _check(self.L.gpis3_sync(self.h), "gpis3_sync")

    def set_pipeline(self, on=True):
        _check(self.L.gpis3_set_pipeline(self.h, int(on)), "gpis3_set_pipeline")

    def set_host_gather(self, on=True):
        _check(self.L.gpis3_set_host_gather(self.h, int(on)), "gpis3_set_host_gather")

    def set_shard_factors(self, mode=-1):
        """Records of a sharded update: 1 factor records (receivers invert lazily), 0 prediction records, -1 follow the inverse mode."""
        _check(self.L.gpis3_set_shard_factors(self.h, int(mode)), "gpis3_set_shard_factors")

    def set_keep_factors(self, on=True):
        """Cross-check switch: keep the training side (factor, re-tiled factor) of every model after its inverse exists."""
        _check(self.L.gpis3_set_keep_factors(self.h, int(on)), "gpis3_set_keep_factors")

    def extract_mesh(self, origin, step, shape, level=None, max_var=None, mesh=None):
        """The map's level surface on the device (gpis3_extract_mesh): test() on the lattice origin + i * step of
        shape (nx, ny, nz), marching tetrahedra at `level` (None: -fbias, the level of the map's surface points), test() on the
        vertices.  Returns (verts [V,3] f32, faces [F,3] i32, rec [V,8] f32); cross(v1 - v0, v2 - v0) points to f >= level.
        max_var drops every face with a vertex whose var_f (rec[:, 4]) is above it and the vertices no face uses.
        mesh: a Mesh to hold the device result (reused across calls; default: one kept by this map)."""
        m = mesh if mesh is not None else self._own_mesh()
        m._extract(self.L.gpis3_extract_mesh, self.h, 3, origin, step, shape, level, "gpis3_extract_mesh")
        v, f, r = m.get()
        return _filter_var(v, f, r, 4, max_var)

    def _own_mesh(self):
        if getattr(self, "_mesh", None) is None:
            self._mesh = Mesh()
        return self._mesh

    def distance_field(self, origin, step, shape, level=None, max_var=None, field=None):
        """The map's signed Euclidean distance field on the device (gpis3_distance_field): test() on the lattice origin + i * step
        of shape (nx, ny, nz) with one step on every axis (a scalar step is accepted), an exact distance transform to the
        level surface (None: -fbias), negative inside (f < level; unknown f counts as outside).  max_var: points whose var_f is
        above it are unknown.  Returns the DistanceField holding the result (field: one to reuse; default: one kept by this map)."""
        df = field if field is not None else self._own_dfield()
        df._compute(self.L.gpis3_distance_field, self.h, self.device(), 3, origin, step, shape, level, max_var, "gpis3_distance_field")
        return df

    def _own_dfield(self):
        if getattr(self, "_dfield", None) is None:
            self._dfield = DistanceField()
        return self._dfield

    def render_depth(self, pose, cam6=None, renderer=None, **opts):
        """What the depth camera would see from `pose` (gpis3_render_depth): rays marched through the map's test() on the device.
        Returns (depth [W*H] f32, rec [W*H, 8] f32, status [W*H] u8) in update()'s column-major layout (k = col * H + row), so
        update(depth, pose) takes the depth.  No hit: depth NaN, record NaN.  Status 0 hit, 1 left the interval, 2 step limit.
        cam6: (fx, fy, cx, cy, width, height), None = the map's camera.  opts: the gpis_render_opts fields (tnear, tfar,
        min_step, max_step, far_step, level, max_var, refine, max_steps).  renderer: a Renderer to hold the device result
        (default: one kept by this map)."""
        pose = np.ascontiguousarray(pose, dtype=np.float32).ravel()
        if pose.size != 12:
            raise GpisError("pose must have 12 elements")
        r = renderer if renderer is not None else self._own_renderer()
        o = render_opts(3, **opts)
        _, cam = _depth_frame("render_depth", None, cam6, self.h, self._wh)
        _check(self.L.gpis3_render_depth(self.h, r.h, cam, _p(pose), C.byref(o), None), "gpis3_render_depth")
        return r.get()

    def _own_renderer(self):
        if getattr(self, "_renderer", None) is None:
            self._renderer = Renderer()
        return self._renderer

    def track_depth(self, depth, pose0, cam6=None, tracker=None, **opts):
        """The camera pose from which the map explains `depth` best (gpis3_track_depth): damped Gauss-Newton on SE(3) from pose0,
        one test() pass over the frame's points per iteration, the normal equations reduced on the device.  depth: [W*H] in
        update()'s column-major layout; pose0: 12 floats [t(3), R(9)].  Returns (pose [12] f32, info): info is Tracker.info()
        plus H [6, 6], b [6] (xi = (v, omega)) at the returned pose and "resid" [W*H] (r of the inliers, NaN elsewhere).
        Non-convergence is info["status"] (0 converged, 1 max_iters, 2 too few inliers, 3 degenerate), not an exception.
        cam6: (fx, fy, cx, cy, width, height), None = the map's camera.  opts: the gpis_track_opts fields."""
        pose0 = np.ascontiguousarray(pose0, dtype=np.float32).ravel()
        if pose0.size != 12:
            raise GpisError("pose must have 12 elements")
        depth, cam = _depth_frame("track_depth", depth, cam6, self.h, self._wh)
        t = tracker if tracker is not None else self._own_tracker()
        o = track_opts(3, **opts)
        out = np.zeros(12, dtype=np.float32)
        _check(self.L.gpis3_track_depth(self.h, t.h, cam, _p(depth), _p(pose0), C.byref(o), _p(out), None), "gpis3_track_depth")
        return out, t.result()

    def _own_tracker(self):
        if getattr(self, "_tracker", None) is None:
            self._tracker = Tracker()
        return self._tracker

    def track_depth_field(self, field, depth, pose0, cam6=None, tracker=None, **opts):
        """track_depth against a DistanceField instead of the map (gpis3_track_depth_field): r = the sampled distance, one
        fused kernel per pass.  cam6 None = this map's camera; nothing else of the map is read.  level and max_var are not
        read (the field's level is zero; its gate was applied when it was built).  Returns (pose, info) as track_depth."""
        return field._track_depth(self.h, self._wh, depth, pose0, cam6, tracker, opts)

    def score_depth_field(self, field, depth, poses, cam6=None, locator=None, **opts):
        """DistanceField.score_depth with this map's camera when cam6 is None (gpis3_locate_depth_field); nothing else of the
        map is read."""
        return field._score_depth(self.h, self._wh, depth, poses, cam6, locator, opts)

    def locate_depth_field(self, field, depth, poses, cam6=None, refine=8, track=None, **opts):
        """DistanceField.locate_depth with this map's camera when cam6 is None."""
        return field._locate(3, (self.h, self._wh, depth, cam6), poses, refine, track, opts)

    def pf_update_depth_field(self, field, pf, depth, cam6=None, stream=None, **opts):
        """ParticleFilter.update_depth with this map's camera when cam6 is None (gpis3_pf_update_depth); nothing else of the
        map is read."""
        return pf._update_depth(self.h, self._wh, field, depth, cam6, stream, opts)

    def cover_depth(self, cover, depth, pose, cam6=None, stream=None, **opts):
        """Coverage.integrate_depth with this map's camera (cam6 None)."""
        return cover._integrate_depth(self.h, self._wh, depth, pose, cam6, stream, opts)

    def view_gain_depth_field(self, field, cover, poses, cam6=None, scorer=None, stream=None, **opts):
        """DistanceField.view_gain_depth with this map's camera when cam6 is None (gpis3_view_gain_depth); nothing else of the
        map is read."""
        return field._view_gain_depth(self.h, cover, cam6, poses, scorer, stream, opts)

    def render_depth_field(self, field, pose, cam6=None, renderer=None, **opts):
        """render_depth from a DistanceField instead of the map (gpis3_render_depth_field): sphere tracing through the field's
        sampler, one fused kernel.  cam6 None = this map's camera; nothing else of the map is read.  Returns (depth [W*H],
        rec [W*H, 4] = (d, gradient), status) as DistanceField.render_depth; opts: the gpis_render_field_opts fields."""
        return field._render_depth(self.h, pose, cam6, renderer, opts)


class GPisMap:
    """Mirror of the reference's mexGPisMap command set ('update', 'test', 'reset') on the HIP path."""

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis2_create())
        if not self.h:
            raise GpisError("gpis2_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis2_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _check(self.L.gpis2_reset(self.h), "gpis2_reset")

    def update(self, thetas, ranges, pose6):
        thetas = np.ascontiguousarray(thetas, dtype=np.float32)
        ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        pose6 = np.ascontiguousarray(pose6, dtype=np.float32)
        if pose6.size != 6 or thetas.size != ranges.size:
            raise GpisError("bad 2-D update arguments")
        _check(self.L.gpis2_update(self.h, _p(thetas), _p(ranges), ranges.size, _p(pose6)), "gpis2_update")

    def test(self, x, res=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        if res is None:
            res = np.zeros((x.shape[0], 6), dtype=np.float32)
        rc = self.L.gpis2_test(self.h, _p(x), 2, x.shape[0], _p(res))
        if rc == -1:
            return None
        _check(rc, "gpis2_test")
        return res

    def test_device(self, d_x_ptr, n, d_res_ptr, stream=0):
        _check(self.L.gpis2_test_device(self.h, C.c_void_p(d_x_ptr), n, C.c_void_p(d_res_ptr), C.c_void_p(stream)),
               "gpis2_test_device")

    def nodes(self):
        n = self.L.gpis2_get_nodes(self.h, None, 0)
        out = np.zeros((n, 7), dtype=np.float32)
        if n:
            self.L.gpis2_get_nodes(self.h, _p(out), n)
        return out

    def stats(self):
        a = (C.c_double * 12)()
        _check(self.L.gpis2_stats(self.h, a, 12), "gpis2_stats")
        return dict(zip(GPisMap3.STAT_KEYS, list(a)))

    def pass_jobs(self):
        """K4 jobs of the last test() per evaluation pass (gpis2_pass_jobs)."""
        a = (C.c_longlong * 4)()
        _check(self.L.gpis2_pass_jobs(self.h, a), "gpis2_pass_jobs")
        return dict(zip(GPisMap3.PASS_KEYS, list(a)))

    def set_pass2_mode(self, mode):
        """As GPisMap3.set_pass2_mode (gpis2_set_pass2_mode)."""
        _check(self.L.gpis2_set_pass2_mode(self.h, int(mode)), "gpis2_set_pass2_mode")

    def pass_detail(self):
        a = (C.c_double * 8)()
        _check(self.L.gpis2_pass_detail(self.h, a), "gpis2_pass_detail")
        return dict(zip(GPisMap3.DETAIL_KEYS, list(a)))

    def sync(self):
        """Join the training the last update() left in flight (pipelined mode); raises when it failed."""
        _check(self.L.gpis2_sync(self.h), "gpis2_sync")

    def set_pipeline(self, on=True):
        _check(self.L.gpis2_set_pipeline(self.h, 1 if on else 0), "gpis2_set_pipeline")

    def extract_contour(self, origin, step, shape, level=None, max_var=None, mesh=None):
        """The map's level contour on the device (gpis2_extract_contour), shape (nx, ny).  Returns (verts [V,2] f32,
        segs [S,2] i32, rec [V,6] f32); the right-hand normal (dy, -dx) of a segment points to f >= level.  max_var: the
        demo's filter on var_f (rec[:, 3])."""
        if mesh is None:
            if getattr(self, "_mesh", None) is None:
                self._mesh = Mesh()
            mesh = self._mesh
        mesh._extract(self.L.gpis2_extract_contour, self.h, 2, origin, step, shape, level, "gpis2_extract_contour")
        v, f, r = mesh.get()
        return _filter_var(v, f, r, 3, max_var)

    def distance_field(self, origin, step, shape, level=None, max_var=None, field=None):
        """The map's signed Euclidean distance field (gpis2_distance_field) on the lattice of shape (nx, ny); as
        GPisMap3.distance_field, var_f = record slot 3."""
        if field is None:
            if getattr(self, "_dfield", None) is None:
                self._dfield = DistanceField()
            field = self._dfield
        field._compute(self.L.gpis2_distance_field, self.h, self.L.gpis2_device(self.h), 2, origin, step, shape, level, max_var, "gpis2_distance_field")
        return field

    def render_scan(self, thetas, pose6, renderer=None, **opts):
        """What the laser would see from `pose6` (gpis2_render_scan) along the beams `thetas`.  Returns (range [n] f32,
        rec [n, 6] f32, status [n] u8); no hit: range NaN, record NaN.  opts: as GPisMap3.render_depth."""
        thetas, _, _ = _scan_frame("render_scan", thetas, None, None, self.h)
        pose6 = np.ascontiguousarray(pose6, dtype=np.float32).ravel()
        if pose6.size != 6:
            raise GpisError("pose6 must have 6 elements")
        if renderer is None:
            if getattr(self, "_renderer", None) is None:
                self._renderer = Renderer()
            renderer = self._renderer
        o = render_opts(2, **opts)
        _check(self.L.gpis2_render_scan(self.h, renderer.h, _p(thetas), thetas.size, _p(pose6), C.byref(o), None),
               "gpis2_render_scan")
        return renderer.get()

    def track_scan(self, thetas, ranges, pose0, tracker=None, **opts):
        """The laser pose from which the map explains the scan best (gpis2_track_scan): damped Gauss-Newton on SE(2) from
        pose0 (6 floats [t(2), R(4)]).  Returns (pose [6] f32, info) with H [3, 3], b [3] (xi = (vx, vy, omega)) and
        "resid" [n]; opts and statuses as GPisMap3.track_depth."""
        thetas, ranges, _ = _scan_frame("track_scan", thetas, ranges, None, self.h)
        pose0 = np.ascontiguousarray(pose0, dtype=np.float32).ravel()
        if pose0.size != 6:
            raise GpisError("pose must have 6 elements")
        if tracker is None:
            if getattr(self, "_tracker", None) is None:
                self._tracker = Tracker()
            tracker = self._tracker
        o = track_opts(2, **opts)
        out = np.zeros(6, dtype=np.float32)
        _check(self.L.gpis2_track_scan(self.h, tracker.h, _p(thetas), _p(ranges), thetas.size, _p(pose0), C.byref(o), _p(out),
                                       None), "gpis2_track_scan")
        return out, tracker.result()

    def track_scan_field(self, field, thetas, ranges, pose0, tracker=None, **opts):
        """track_scan against a DistanceField instead of the map (gpis2_track_scan_field), with this map's sensor offset;
        opts and the result as GPisMap3.track_depth_field."""
        return field._track_scan(self.h, thetas, ranges, pose0, None, tracker, opts)

    def score_scan_field(self, field, thetas, ranges, poses, locator=None, **opts):
        """DistanceField.score_scan with this map's sensor offset (gpis2_locate_scan_field); nothing else of the map is read."""
        return field._score_scan(self.h, thetas, ranges, poses, None, locator, opts)

    def locate_scan_field(self, field, thetas, ranges, poses, refine=8, track=None, **opts):
        """DistanceField.locate_scan with this map's sensor offset."""
        return field._locate(2, (self.h, thetas, ranges, None), poses, refine, track, opts)

    def pf_update_scan_field(self, field, pf, thetas, ranges, stream=None, **opts):
        """ParticleFilter.update_scan with this map's sensor offset (gpis2_pf_update_scan); nothing else of the map is read."""
        return pf._update_scan(self.h, field, thetas, ranges, None, stream, opts)

    def cover_scan(self, cover, thetas, ranges, pose6, off2=None, stream=None, **opts):
        """Coverage.integrate_scan with this map's sensor offset (off2 None)."""
        return cover._integrate_scan(self.h, thetas, ranges, pose6, off2, stream, opts)

    def view_gain_scan_field(self, field, cover, thetas, poses, off2=None, scorer=None, stream=None, **opts):
        """DistanceField.view_gain_scan with this map's sensor offset when off2 is None (gpis2_view_gain_scan); nothing else of
        the map is read."""
        return field._view_gain_scan(self.h, cover, thetas, poses, off2, scorer, stream, opts)

    def render_scan_field(self, field, thetas, pose6, renderer=None, **opts):
        """render_scan from a DistanceField instead of the map (gpis2_render_scan_field), with this map's sensor offset;
        opts and the result as DistanceField.render_scan."""
        return field._render_scan(self.h, thetas, pose6, None, renderer, opts)


def _filter_var(verts, prims, rec, slot, max_var):
    """Drop every primitive with a vertex whose variance (rec[:, slot]) is above max_var, then the vertices no primitive uses
    (order kept, primitives renumbered)."""
    if max_var is None:
        return verts, prims, rec
    keep = np.all(rec[prims, slot] <= np.float32(max_var), axis=1) if prims.size else np.zeros(0, bool)
    prims = prims[keep]
    used = np.zeros(verts.shape[0], bool)
    used[prims.ravel()] = True
    remap = np.cumsum(used, dtype=np.int64) - 1
    return verts[used], remap[prims].astype(np.int32), rec[used]


class Mesh:
    """Result holder of the surface extraction (gpis_mesh_*): device buffers reused across calls.  Kernel level:
    from_grid() on any device-resident value grid."""

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_mesh_create())
        if not self.h:
            raise GpisError("gpis_mesh_create failed")
        self.dim = 0
        self.shape = None

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_mesh_destroy(self.h)
            self.h = None

    __del__ = close

    def set_chunk(self, points):
        """Lattice points per test() pass of a map-level extraction (0 = default 2^22; results do not depend on it)."""
        _check(self.L.gpis_mesh_set_chunk(self.h, int(points)), "gpis_mesh_set_chunk")

    @staticmethod
    def _lattice_args(dim, origin, step, shape):
        n = np.ascontiguousarray(shape, dtype=np.int32).ravel()
        o = np.ascontiguousarray(origin, dtype=np.float32).ravel()
        s = np.ascontiguousarray(step if np.ndim(step) else [step] * dim, dtype=np.float32).ravel()
        if n.size != dim or o.size != dim or s.size != dim:
            raise GpisError("lattice arguments must have %d entries" % dim)
        return n, o, s

    def _extract(self, fn, map_h, dim, origin, step, shape, level, what):
        n, o, s = self._lattice_args(dim, origin, step, shape)
        lv = float("nan") if level is None else float(level)
        _check(fn(map_h, self.h, _p(n, C.c_int), _p(o), _p(s), lv, None), what)
        self.dim, self.shape = dim, tuple(int(v) for v in n)

    def from_grid(self, d_val_ptr, shape, origin, step, level, stream=0):
        """Kernel level (gpis_mesh_from_grid): d_val_ptr = device address of prod(shape) float32 values, x fastest."""
        dim = len(shape)
        n, o, s = self._lattice_args(dim, origin, step, shape)
        _check(self.L.gpis_mesh_from_grid(self.h, C.c_void_p(d_val_ptr), dim, _p(n, C.c_int), _p(o), _p(s), float(level),
                                          C.c_void_p(stream)), "gpis_mesh_from_grid")
        self.dim, self.shape = dim, tuple(int(v) for v in n)

    def counts(self):
        nv, npr = C.c_longlong(0), C.c_longlong(0)
        _check(self.L.gpis_mesh_counts(self.h, C.byref(nv), C.byref(npr)), "gpis_mesh_counts")
        return int(nv.value), int(npr.value)

    def get(self, records=None):
        """(verts [V,dim], prims [P,dim], rec [V,2(1+dim)] or None): host copies of the last result."""
        nv, npr = self.counts()
        d = max(self.dim, 2)
        v = np.zeros((nv, d), dtype=np.float32)
        p = np.zeros((npr, d), dtype=np.int32)
        want = self.has_records() if records is None else records
        r = np.zeros((nv, 2 * (1 + d)), dtype=np.float32) if want else None
        _check(self.L.gpis_mesh_get(self.h, _p(v), _p(p, C.c_int), _p(r) if r is not None else None), "gpis_mesh_get")
        return v, p, r

    def has_records(self):
        dv = C.c_void_p(0)
        _check(self.L.gpis_mesh_device(self.h, None, None, C.byref(dv)), "gpis_mesh_device")
        return bool(dv.value)

    def grid(self):
        """The value grid (f) of the last map-level extraction, shape[::-1] (x fastest)."""
        out = np.zeros(int(np.prod(self.shape)), dtype=np.float32)
        _check(self.L.gpis_mesh_get_grid(self.h, _p(out)), "gpis_mesh_get_grid")
        return out.reshape(self.shape[::-1])

    def device_ptrs(self):
        a, b, c = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_mesh_device(self.h, C.byref(a), C.byref(b), C.byref(c)), "gpis_mesh_device")
        return a.value or 0, b.value or 0, c.value or 0


class DistanceField:
    """Result holder of the signed distance field (gpis_dfield_*): device buffers reused across calls.  Kernel level:
    from_grid() on any device-resident f grid.  get() -> (dist, site, f), sample() -> interpolated distance and gradient."""

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_dfield_create())
        if not self.h:
            raise GpisError("gpis_dfield_create failed")
        self._device = get_device()

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_dfield_destroy(self.h)
            self.h = None

    __del__ = close

    def set_chunk(self, points):
        """Lattice points per test() pass of a map-level call (0 = default 2^22; results do not depend on it)."""
        _check(self.L.gpis_dfield_set_chunk(self.h, int(points)), "gpis_dfield_set_chunk")

    def _compute(self, fn, map_h, map_dev, dim, origin, step, shape, level, max_var, what):
        n, o, s = Mesh._lattice_args(dim, origin, step, shape)
        lv = float("nan") if level is None else float(level)
        mv = float("inf") if max_var is None else float(max_var)
        rc = fn(map_h, self.h, _p(n, C.c_int), _p(o), _p(s), lv, mv, None)
        if rc == 0:                                     # (the buffers now live on the map's lead device)
            self._device = map_dev
        _check(rc, what)

    def from_grid(self, d_val_ptr, shape, origin, step, level, stream=0):
        """Kernel level (gpis_dfield_from_grid): d_val_ptr = device address of prod(shape) float32 values, x fastest."""
        dim = len(shape)
        n, o, s = Mesh._lattice_args(dim, origin, step, shape)
        _check(self.L.gpis_dfield_from_grid(self.h, C.c_void_p(d_val_ptr), dim, _p(n, C.c_int), _p(o), _p(s), float(level),
                                            C.c_void_p(stream)), "gpis_dfield_from_grid")
        return self

    def info(self):
        """dict(dim, shape, origin, step) of the last result (dim 0: none)."""
        d, n = C.c_int(0), np.zeros(3, np.int32)
        o, s = np.zeros(3, np.float32), C.c_float(0)
        _check(self.L.gpis_dfield_info(self.h, C.byref(d), _p(n, C.c_int), _p(o), C.byref(s)), "gpis_dfield_info")
        dim = int(d.value)
        return dict(dim=dim, shape=tuple(int(v) for v in n[:dim]), origin=tuple(float(v) for v in o[:dim]), step=float(s.value))

    def get(self, f=None):
        """(dist, site, f) host copies of the last result, each of shape shape[::-1] (x fastest); f is None after from_grid
        (f=True demands it)."""
        inf = self.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        shape = inf["shape"][::-1]
        n = int(np.prod(shape))
        want_f = self.device_ptrs()[2] != 0 if f is None else bool(f)
        dist = np.zeros(n, np.float32)
        site = np.zeros(n, np.int32)
        fv = np.zeros(n, np.float32) if want_f else None
        _check(self.L.gpis_dfield_get(self.h, _p(dist), _p(site, C.c_int), _p(fv) if fv is not None else None), "gpis_dfield_get")
        return dist.reshape(shape), site.reshape(shape), (fv.reshape(shape) if fv is not None else None)

    def device_ptrs(self):
        """(d_dist, d_site, d_f) device addresses of the last result (0 where there is none)."""
        a, b, c = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_dfield_device(self.h, C.byref(a), C.byref(b), C.byref(c)), "gpis_dfield_device")
        return a.value or 0, b.value or 0, c.value or 0

    def sample(self, points, m=None, d_out=None, stream=0):
        """Interpolated distance and gradient (gpis_dfield_sample).  points: a numpy [m, dim] array -> returns [m, 1 + dim]
        float32; or a device address of m * dim floats with d_out the device address of m * (1 + dim) floats (returns None).
        Points outside the lattice give NaN."""
        if isinstance(points, int):
            if m is None or d_out is None:
                raise GpisError("sample on a device pointer needs m and d_out")
            _check(self.L.gpis_dfield_sample(self.h, C.c_void_p(points), int(m), C.c_void_p(d_out), C.c_void_p(stream)),
                   "gpis_dfield_sample")
            return None
        import torch
        dim = self.info()["dim"]
        if dim == 0:
            raise GpisError("distance field holds no result")
        x = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, dim)
        dev = torch.device("cuda", self.device())
        tx = torch.from_numpy(x).to(dev)
        to = torch.empty((x.shape[0], 1 + dim), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        _check(self.L.gpis_dfield_sample(self.h, C.c_void_p(tx.data_ptr()), x.shape[0], C.c_void_p(to.data_ptr()), None),
               "gpis_dfield_sample")
        return to.cpu().numpy()

    def device(self):
        """The HIP device the buffers live on (the one current at creation; a map-level call moves them to the map's lead
        device)."""
        return self._device

    def track_depth(self, depth, pose0, cam6, tracker=None, **opts):
        """The camera pose from which this field explains `depth` best (gpis3_track_depth_field without a map): track_depth's
        Gauss-Newton with r = the sampled distance, one fused kernel per pass.  cam6: (fx, fy, cx, cy, width, height).  level
        and max_var are not read.  Returns (pose [12] f32, info) as GPisMap3.track_depth."""
        return self._track_depth(None, None, depth, pose0, cam6, tracker, opts)

    def track_scan(self, thetas, ranges, pose0, off2, tracker=None, **opts):
        """The laser pose from which this field explains the scan best (gpis2_track_scan_field without a map); off2: the
        sensor offset (x, y) in the laser frame.  Returns (pose [6] f32, info) as GPisMap.track_scan."""
        return self._track_scan(None, thetas, ranges, pose0, off2, tracker, opts)

    def _own_tracker(self):
        if getattr(self, "_tracker", None) is None:
            self._tracker = Tracker()
        return self._tracker

    def _track_depth(self, map_h, map_wh, depth, pose0, cam6, tracker, opts):
        pose0 = np.ascontiguousarray(pose0, dtype=np.float32).ravel()
        if pose0.size != 12:
            raise GpisError("pose must have 12 elements")
        depth, cam = _depth_frame("track_depth", depth, cam6, map_h, map_wh)
        t = tracker if tracker is not None else self._own_tracker()
        o = track_opts(3, **opts)
        out = np.zeros(12, dtype=np.float32)
        _check(self.L.gpis3_track_depth_field(map_h, self.h, t.h, cam, _p(depth), _p(pose0), C.byref(o), _p(out), None),
               "gpis3_track_depth_field")
        return out, t.result()

    def _track_scan(self, map_h, thetas, ranges, pose0, off2, tracker, opts):
        thetas, ranges, off = _scan_frame("track_scan", thetas, ranges, off2, map_h)
        pose0 = np.ascontiguousarray(pose0, dtype=np.float32).ravel()
        if pose0.size != 6:
            raise GpisError("pose must have 6 elements")
        t = tracker if tracker is not None else self._own_tracker()
        o = track_opts(2, **opts)
        out = np.zeros(6, dtype=np.float32)
        _check(self.L.gpis2_track_scan_field(map_h, self.h, t.h, _p(thetas), _p(ranges), thetas.size, off, _p(pose0), C.byref(o),
                                             _p(out), None), "gpis2_track_scan_field")
        return out, t.result()

    def score_depth(self, depth, poses, cam6, locator=None, **opts):
        """Which of `poses` [m, 12] (float32 [t(3), R(9)]) explains `depth` against this field (gpis3_locate_depth_field without
        a map): per pose the truncated sum of squared field distances of the tracker's points, one wavefront per pose in one
        kernel.  Returns (cost [m] f64, inliers [m] i32, order [min(top_k, m)] i32: cost ascending, ties by the lower index).
        opts: the gpis_locate_opts fields (max_residual, stride, top_k; top_k=0 ranks all).  locator: a Locator to hold the
        device result (default: one kept by this field)."""
        return self._score_depth(None, None, depth, poses, cam6, locator, opts)

    def score_scan(self, thetas, ranges, poses, off2, locator=None, **opts):
        """Which of `poses` [m, 6] (float32 [t(2), R(4)]) explains the scan against this field (gpis2_locate_scan_field without a
        map); off2: the sensor offset (x, y) in the laser frame.  Returns (cost, inliers, order) as score_depth."""
        return self._score_scan(None, thetas, ranges, poses, off2, locator, opts)

    def locate_depth(self, depth, poses, cam6, refine=8, track=None, **opts):
        """Locate and refine: score `poses` (score_depth with opts), run the field tracker (track_depth with the options in
        `track`) from each of the first `refine` ranked poses, score the refined poses in a second call with the same options
        and return the one of the lowest cost (ties: the better first rank).  Returns (pose [12] f32, info): info holds the
        first ranking ("cost", "inliers", "order"), "candidates" (the ranked indices refined), "tracks" (their tracker infos),
        "refined" [r, 12], "refined_cost", "refined_inliers" and "best" (the index into the candidates).  refine=0 returns the
        best-ranked pose itself."""
        return self._locate(3, (None, None, depth, cam6), poses, refine, track, opts)

    def locate_scan(self, thetas, ranges, poses, off2, refine=8, track=None, **opts):
        """locate_depth for a laser scan: score_scan, track_scan from the first `refine` ranked poses, score_scan again."""
        return self._locate(2, (None, thetas, ranges, off2), poses, refine, track, opts)

    def _own_locator(self):
        if getattr(self, "_locator", None) is None:
            self._locator = Locator()
        return self._locator

    def _score_depth(self, map_h, map_wh, depth, poses, cam6, locator, opts):
        poses = np.ascontiguousarray(poses, dtype=np.float32)
        if poses.size == 0 or poses.size % 12:
            raise GpisError("poses must be [m, 12] with m >= 1")
        depth, cam = _depth_frame("score_depth", depth, cam6, map_h, map_wh)
        l = locator if locator is not None else self._own_locator()
        o = locate_opts(3, **opts)
        _check(self.L.gpis3_locate_depth_field(map_h, self.h, l.h, cam, _p(depth), _p(poses), poses.size // 12, C.byref(o), None),
               "gpis3_locate_depth_field")
        return l.get()

    def _score_scan(self, map_h, thetas, ranges, poses, off2, locator, opts):
        poses = np.ascontiguousarray(poses, dtype=np.float32)
        if poses.size == 0 or poses.size % 6:
            raise GpisError("poses must be [m, 6] with m >= 1")
        thetas, ranges, off = _scan_frame("score_scan", thetas, ranges, off2, map_h)
        l = locator if locator is not None else self._own_locator()
        o = locate_opts(2, **opts)
        _check(self.L.gpis2_locate_scan_field(map_h, self.h, l.h, _p(thetas), _p(ranges), thetas.size, off, _p(poses),
                                              poses.size // 6, C.byref(o), None), "gpis2_locate_scan_field")
        return l.get()

    def _locate(self, dim, frame, poses, refine, track, opts):
        np_ = 12 if dim == 3 else 6
        poses = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, np_)
        if dim == 3:
            map_h, map_wh, depth, cam6 = frame
            score = lambda P: self._score_depth(map_h, map_wh, depth, P, cam6, None, opts)
            polish = lambda P: self._track_depth(map_h, map_wh, depth, P, cam6, None, dict(track or {}))
        else:
            map_h, thetas, ranges, off2 = frame
            score = lambda P: self._score_scan(map_h, thetas, ranges, P, off2, None, opts)
            polish = lambda P: self._track_scan(map_h, thetas, ranges, P, off2, None, dict(track or {}))
        cost, inliers, order = score(poses)
        cand = order[:max(0, int(refine))]
        info = dict(cost=cost, inliers=inliers, order=order, candidates=cand, tracks=[], refined=None, refined_cost=None,
                    refined_inliers=None, best=0)
        if cand.size == 0:
            return poses[order[0]].copy(), info
        refined = np.zeros((cand.size, np_), np.float32)
        for k, i in enumerate(cand):
            refined[k], t = polish(poses[i])
            info["tracks"].append(t)
        c2, n2, _ = score(refined)
        best = int(np.argmin(c2))                       # (the first of equal costs: the better first rank)
        info.update(refined=refined, refined_cost=c2, refined_inliers=n2, best=best)
        return refined[best].copy(), info

    def render_depth(self, pose, cam6, renderer=None, **opts):
        """What a depth camera at `pose` would see of this field (gpis3_render_depth_field without a map): every ray sphere-traced
        through the sampler in one thread of one kernel.  cam6: (fx, fy, cx, cy, width, height).  Returns (depth [W*H] f32,
        rec [W*H, 4] f32 = (d, gradient) at the reported point, status [W*H] u8) in update()'s column-major layout; no hit:
        NaN.  Status 0 hit, 1 left the interval, 2 step limit.  opts: the gpis_render_field_opts fields (tnear, tfar, min_step,
        max_step, slack, refine, max_steps; defaults for this field's step).  A step clamped up to min_step (default half a
        cell) can pass through anything thinner.  renderer: a Renderer to hold the device result (default: one kept by this
        field)."""
        return self._render_depth(None, pose, cam6, renderer, opts)

    def render_scan(self, thetas, pose6, off2, renderer=None, **opts):
        """What a laser at `pose6` would see of this field along the beams `thetas` (gpis2_render_scan_field without a map);
        off2: the sensor offset (x, y) in the laser frame.  Returns (range [n], rec [n, 3], status [n])."""
        return self._render_scan(None, thetas, pose6, off2, renderer, opts)

    def _own_renderer(self):
        if getattr(self, "_renderer", None) is None:
            self._renderer = Renderer()
        return self._renderer

    def detect_scan(self, thetas, ranges, pose, off2, t, detector=None, cover=None, obstacles=None, stream=None, **opts):
        """Moving obstacles of a laser scan (gpis2_detect_scan_field without a map): the beams that end in what this field holds
        as free space, at least min_dist from every surface, grouped along the scan into components and turned into one ball
        each, with velocities from the detector's tracks.  pose [6] in double ([t(2), R(4)]); t: the absolute time of the scan;
        cover: a Coverage of this field's lattice (a sample counts only where the mask is set); obstacles: an Obstacles set to
        receive the balls (Detector.to_obstacles).  opts: the gpis_detect_opts fields.  Returns Detector.result()."""
        thetas, ranges, off = _scan_frame("detect_scan", thetas, ranges, off2, None)
        pose = np.ascontiguousarray(pose, dtype=np.float64).ravel()
        if pose.size != 6:
            raise GpisError("pose must have 6 elements")
        d = detector if detector is not None else self._own_detector()
        o = self._detect_opts(2, opts)
        _check(self.L.gpis2_detect_scan_field(None, self.h, d.h, cover.h if cover is not None else None, _p(thetas), _p(ranges),
                                              thetas.size, off, _p(pose, C.c_double), float(t), o, C.c_void_p(stream or 0)),
               "gpis2_detect_scan_field")
        if obstacles is not None:
            d.to_obstacles(obstacles)
        return d.result()

    def detect_depth(self, depth, pose, cam6, t, detector=None, cover=None, obstacles=None, stream=None, **opts):
        """detect_scan for a depth frame (gpis3_detect_depth_field without a map): the tracker's strided pixels, components
        over the 8 neighbours on the strided grid.  pose [12] in double ([t(3), R(9)]); cam6: (fx, fy, cx, cy, width, height)."""
        depth, cam = _depth_frame("detect_depth", depth, cam6, None, None)
        pose = np.ascontiguousarray(pose, dtype=np.float64).ravel()
        if pose.size != 12:
            raise GpisError("pose must have 12 elements")
        d = detector if detector is not None else self._own_detector()
        o = self._detect_opts(3, opts)
        _check(self.L.gpis3_detect_depth_field(None, self.h, d.h, cover.h if cover is not None else None, cam, _p(depth),
                                               _p(pose, C.c_double), float(t), o, C.c_void_p(stream or 0)),
               "gpis3_detect_depth_field")
        if obstacles is not None:
            d.to_obstacles(obstacles)
        return d.result()

    def _detect_opts(self, dim, opts):
        # (a field without a result has no step: the entry itself refuses it, with GPIS_ERR_STATE)
        step = self.info()["step"]
        return C.byref(detect_opts(dim, step, **opts)) if step > 0 else None

    def _own_detector(self):
        if getattr(self, "_detector", None) is None:
            self._detector = Detector()
        return self._detector

    def plan(self, goals, planner=None, **opts):
        """Cost-to-go and policy over this field's free space towards `goals` [g, dim] (gpis_plan_solve).  opts: the
        gpis_plan_opts fields (clearance, margin, gain, connectivity, max_rounds; defaults for this field's step).  Unknown
        space is outside in the field and therefore free.  Returns the Planner holding the result (default: one kept by this
        field); it stays valid when the field is recomputed."""
        p = planner if planner is not None else self._own_planner()
        return p.solve(self, goals, **opts)

    def plan_timed(self, goals, obstacles=None, t_begin=0.0, time_planner=None, **opts):
        """A plan through space and time over this 2-D field's free space towards `goals` [g, 2] around the moving balls of
        `obstacles` (an Obstacles, or None) from absolute time t_begin on (gpis_tplan_solve).  opts: the gpis_tplan_opts fields
        (clearance, margin, gain, connectivity, slot, horizon, dyn_clearance, wait, keep_cost).  Returns the TimePlanner holding
        the result (default: one kept by this field); it stays valid when the field or the set changes."""
        if time_planner is None:
            if getattr(self, "_time_planner", None) is None:
                self._time_planner = TimePlanner()
            time_planner = self._time_planner
        return time_planner.solve(self, goals, obstacles, t_begin, **opts)

    def plan_poses_timed(self, goals, footprint, obstacles=None, H=16, moves="any", t_begin=0.0, time_pose_planner=None, **opts):
        """A plan through space and time over poses (x, y, heading index) of this 2-D field for `footprint` towards `goals`
        [g, 3] or [g, 2] around the moving balls of `obstacles` (an Obstacles, or None) from absolute time t_begin on
        (gpis_tpplan_solve): every body ball keeps dyn_clearance from every moving ball during every move.  H, moves: as
        plan_poses (heading_table, heading_moves).  opts: the gpis_tpplan_opts fields (clearance, margin, gain, turn, slot,
        horizon, dyn_clearance, wait, keep_cost).  Returns the TimePosePlanner holding the result (default: one kept by this
        field); it stays valid when the field, the set or the footprint changes."""
        if time_pose_planner is None:
            if getattr(self, "_time_pose_planner", None) is None:
                self._time_pose_planner = TimePosePlanner()
            time_pose_planner = self._time_pose_planner
        return time_pose_planner.solve(self, goals, footprint, obstacles, H=H, moves=moves, t_begin=t_begin, **opts)

    def plan_poses(self, footprint, goals, H=16, moves="any", pose_planner=None, **opts):
        """Cost-to-go and policy over poses (x, y, heading index) of this 2-D field for `footprint` towards `goals` [g, 3] or
        [g, 2] (gpis_pplan_solve): routes the body fits through, where plan() routes a point.  opts: the gpis_pplan_opts
        fields (clearance, margin, gain, turn, max_rounds).  Returns the PosePlanner holding the result (default: one kept by
        this field); its project() gives a Planner for the consumers of plan()."""
        if pose_planner is None:
            if getattr(self, "_pose_planner", None) is None:
                self._pose_planner = PosePlanner()
            pose_planner = self._pose_planner
        return pose_planner.solve(self, footprint, goals, H=H, moves=moves, **opts)

    def _own_planner(self):
        if getattr(self, "_planner", None) is None:
            self._planner = Planner()
        return self._planner

    def smooth(self, x_or_planner, N=64, trajectories=None, stream=0, footprint=None, w_turn=None, **opts):
        """Trajectories through this field (gpis_traj_*): the last paths of a Planner (or the points of a PosePlanner's)
        resampled to N waypoints each, or the caller's waypoints [m, N, dim], run through the covariant gradient descent and
        evaluated.  opts: the gpis_traj_opts fields (clearance, margin, w_smooth, w_obs, rate, max_move, tol, iters, sub;
        defaults for this field's step); iters=0 is the collision check alone.  footprint, w_turn: Trajectories.optimize's
        (smoothing for the body, gpis_smooth_body_optimize).  Returns the Trajectories holding the result (default: one kept by
        this field); it stays valid when the field is recomputed."""
        t = trajectories if trajectories is not None else self._own_trajectories()
        if isinstance(x_or_planner, Planner):
            t.from_paths(x_or_planner, N)
        elif isinstance(x_or_planner, PosePlanner):
            t.from_pose_paths(x_or_planner, N)
        else:
            t.set(x_or_planner)
        return t.optimize(self, footprint=footprint, w_turn=w_turn, stream=stream, **opts)

    def _own_trajectories(self):
        if getattr(self, "_trajectories", None) is None:
            self._trajectories = Trajectories()
        return self._trajectories

    def control(self, controller, pose, goal=None, planner=None, stream=None, obstacles=None, t=0.0, footprint=None, **opts):
        """One step of a sampling Controller through this field (gpis_mppi_step): pose [t, R] as a filter's estimate returns
        it; exactly one of `goal` (a point [dim]) and `planner` (a Planner solved on this field's lattice) gives the terminal
        cost.  opts: the gpis_mppi_opts fields (`lam` for lambda; defaults for this field's step).  Returns (u0, info): the
        first control of the new nominal sequence and dict(Jmin, best, neff, hits, nominal_cost, nominal_hits, T, Th, S2).
        obstacles: an Obstacles whose balls, moved to the absolute time t of `pose` and on from there, are charged in every
        rollout (gpis_obst_mppi_step); None keeps the plain step.  footprint: a Footprint whose balls, placed at every rollout
        state, stand in for the point (gpis_body_mppi_step); None or an empty one keeps the point."""
        return controller.step(self, pose, goal=goal, planner=planner, stream=stream, obstacles=obstacles, t=t, footprint=footprint, **opts)

    def body_clearance(self, footprint, states, clearance=0.0, stream=None):
        """Footprint.clearance on this field."""
        return footprint.clearance(self, states, clearance=clearance, stream=stream)

    def explore(self, cover, start, planner=None, out=None, unseen_dist=None, **opts):
        """Where to go next to see more: the frontiers of `cover` (a Coverage on this field's lattice), this field restricted to
        seen space, a plan on the restricted field with the cluster representatives as goals, and the path from `start`
        [dim].  opts: the gpis_plan_opts fields plus the coverage's min_size; `clearance` (default the coverage's, 3 steps) is
        shared by the frontiers and the planner, max_rounds is the planner's.  Returns (path [len, dim] f32, status,
        clusters): the planner's path status, or 4 and an empty path when there is no frontier; clusters as
        Coverage.frontiers.  A composition of calls that exist: no device code of its own."""
        copts = {k: opts.pop(k) for k in ("min_size", "back_off", "max_gap") if k in opts}
        if "clearance" in opts:
            copts["clearance"] = opts["clearance"]
        clusters = cover.frontiers(self, **copts)
        dim = self.info()["dim"]
        if clusters["label"].size == 0:
            return np.zeros((0, dim), np.float32), 4, clusters
        opts.setdefault("clearance", cover_opts(dim, self._step()).clearance)
        r = cover.restrict(self, out=out, unseen_dist=unseen_dist)
        p = planner if planner is not None else self._own_planner()
        p.solve(r, clusters["rep"], **opts)
        paths, _, status = p.paths(np.ascontiguousarray(start, dtype=np.float32).reshape(1, dim))
        return paths[0], int(status[0]), clusters

    def view_gain_depth(self, cover, cam6, poses, scorer=None, stream=None, **opts):
        """How much unseen space a depth camera would reveal from each of `poses` [m, 12] (gpis3_view_gain_depth without a map):
        per pose the field renderer's prediction of the frame, rays without a return measured as `miss`, and the number of
        points of `cover` (a Coverage on this field's lattice) that integrating that frame would newly see, among those with
        !(dist < min_dist).  Neither the field nor the mask changes.  opts: the gpis_view_opts fields (back_off, max_gap, miss,
        min_dist) and the march's (gpis_render_field_opts).  scorer: a ViewScorer to hold the result (default: one kept by this
        field).  Returns (gain int64 [m], hits int32 [m])."""
        return self._view_gain_depth(None, cover, cam6, poses, scorer, stream, opts)

    def view_gain_scan(self, cover, thetas, poses, off2, scorer=None, stream=None, **opts):
        """view_gain_depth for a laser with beams `thetas` at each of `poses` [m, 6] (gpis2_view_gain_scan without a map); off2:
        the sensor offset (x, y) in the laser frame."""
        return self._view_gain_scan(None, cover, thetas, poses, off2, scorer, stream, opts)

    def _own_scorer(self):
        if getattr(self, "_scorer", None) is None:
            self._scorer = ViewScorer()
        return self._scorer

    def _view_gain_depth(self, map_h, cover, cam6, poses, scorer, stream, opts):
        poses = np.ascontiguousarray(poses, dtype=np.float32)
        if poses.size == 0 or poses.size % 12:
            raise GpisError("poses must be [m, 12] with m >= 1")
        _, cam = _depth_frame("view_gain_depth", None, cam6, map_h, None)
        v = scorer if scorer is not None else self._own_scorer()
        o = view_opts(3, self._step(), **opts)
        _check(self.L.gpis3_view_gain_depth(map_h, self.h, cover.h, v.h, cam, _p(poses), poses.size // 12, C.byref(o),
                                            C.c_void_p(stream or 0)), "gpis3_view_gain_depth")
        return v.get()

    def _view_gain_scan(self, map_h, cover, thetas, poses, off2, scorer, stream, opts):
        thetas, _, off = _scan_frame("view_gain_scan", thetas, None, off2, map_h)
        poses = np.ascontiguousarray(poses, dtype=np.float32)
        if poses.size == 0 or poses.size % 6:
            raise GpisError("poses must be [m, 6] with m >= 1")
        v = scorer if scorer is not None else self._own_scorer()
        o = view_opts(2, self._step(), **opts)
        _check(self.L.gpis2_view_gain_scan(map_h, self.h, cover.h, v.h, _p(thetas), thetas.size, off, _p(poses), poses.size // 6,
                                           C.byref(o), C.c_void_p(stream or 0)), "gpis2_view_gain_scan")
        return v.get()

    def next_view(self, cover, start, sensor, yaws, base_pose=None, planner=None, out=None, unseen_dist=None, scorer=None, **opts):
        """Which way to look next, and how to get there: the frontiers of `cover`, one candidate pose per (cluster representative,
        yaw), the candidates scored by view_gain_*, the pose of largest gain (ties to the lowest index), and the path from
        `start` to its representative through this field restricted to seen space, as explore plans it.  sensor: 2-D
        (thetas, off2), 3-D cam6.  2-D candidates: pose_grid2 at the representative; 3-D: pose_grid3 around `base_pose` [12]
        moved to the representative, rotation vectors (0, 0, yaw).  opts: explore's (the gpis_plan_opts fields, min_size) and
        the gpis_view_opts fields with the march's.  Returns (path, status, pose, gains, clusters): the planner's status, or 4
        with an empty path and a None pose when there is no cluster or every gain is 0; gains int64 [clusters, yaws].  A
        composition of calls that exist: no device code of its own."""
        dim = self.info()["dim"]
        vnames = {f[0] for f in gpis_view_opts._fields_ + gpis_render_field_opts._fields_} - {"march"}
        vopts = {k: opts.pop(k) for k in list(opts) if k in vnames}
        copts = {k: opts.pop(k) for k in ("min_size",) if k in opts}
        if "clearance" in opts:
            copts["clearance"] = opts["clearance"]
        clusters = cover.frontiers(self, **copts)
        yaws = np.atleast_1d(np.asarray(yaws, dtype=np.float64))
        nc = clusters["label"].size
        empty = np.zeros((0, dim), np.float32)
        if nc == 0 or yaws.size == 0:
            return empty, 4, None, np.zeros((nc, yaws.size), np.int64), clusters
        rep = clusters["rep"]
        if dim == 2:
            thetas, off2 = sensor
            poses = np.concatenate([pose_grid2([r[0]], [r[1]], yaws) for r in rep])
            gains, _ = self.view_gain_scan(cover, thetas, poses, off2, scorer=scorer, **vopts)
        else:
            if base_pose is None:
                raise GpisError("a 3-D next_view needs base_pose")
            base = np.ascontiguousarray(base_pose, dtype=np.float32).ravel().copy()
            rv = np.stack([np.zeros_like(yaws), np.zeros_like(yaws), yaws], axis=1)
            parts = []
            for r in rep:
                base[:3] = r
                parts.append(pose_grid3(base, np.zeros((1, 3)), rv))
            poses = np.concatenate(parts)
            gains, _ = self.view_gain_depth(cover, sensor, poses, scorer=scorer, **vopts)
        best = int(np.argmax(gains))                        # (the first maximum: the lowest index)
        gains = gains.reshape(nc, yaws.size)
        if gains.ravel()[best] == 0:
            return empty, 4, None, gains, clusters
        opts.setdefault("clearance", cover_opts(dim, self._step()).clearance)
        r = cover.restrict(self, out=out, unseen_dist=unseen_dist)
        p = planner if planner is not None else self._own_planner()
        p.solve(r, rep[best // yaws.size].reshape(1, dim), **opts)
        paths, _, status = p.paths(np.ascontiguousarray(start, dtype=np.float32).reshape(1, dim))
        return paths[0], int(status[0]), poses.reshape(-1, 12 if dim == 3 else 6)[best].copy(), gains, clusters

    def _step(self):
        inf = self.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        return inf["step"]

    def _render_depth(self, map_h, pose, cam6, renderer, opts):
        pose = np.ascontiguousarray(pose, dtype=np.float32).ravel()
        if pose.size != 12:
            raise GpisError("pose must have 12 elements")
        _, cam = _depth_frame("render_depth", None, cam6, map_h, None)
        r = renderer if renderer is not None else self._own_renderer()
        o = render_field_opts(3, self._step(), **opts)
        _check(self.L.gpis3_render_depth_field(map_h, self.h, r.h, cam, _p(pose), C.byref(o), None), "gpis3_render_depth_field")
        return r.get()

    def _render_scan(self, map_h, thetas, pose6, off2, renderer, opts):
        thetas, _, off = _scan_frame("render_scan", thetas, None, off2, map_h)
        pose6 = np.ascontiguousarray(pose6, dtype=np.float32).ravel()
        if pose6.size != 6:
            raise GpisError("pose6 must have 6 elements")
        r = renderer if renderer is not None else self._own_renderer()
        o = render_field_opts(2, self._step(), **opts)
        _check(self.L.gpis2_render_scan_field(map_h, self.h, r.h, _p(thetas), thetas.size, off, _p(pose6), C.byref(o), None),
               "gpis2_render_scan_field")
        return r.get()


def plan_opts(dim, step, **opts):
    """gpis_plan_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_plan_default_opts) with the
    given fields replaced."""
    o = gpis_plan_opts()
    _check(lib().gpis_plan_default_opts(int(dim), float(step), C.byref(o)), "gpis_plan_default_opts")
    names = {f[0] for f in gpis_plan_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown plan option %r" % k)
        setattr(o, k, v)
    return o


class Planner:
    """Result holder of the path planner (gpis_plan_*): cost-to-go, policy and paths on the device, buffers reused across
    calls.  A finished plan does not depend on the field it was solved on."""

    INFO_KEYS = ("valid", "dim", "nx", "ny", "nz", "step", "goals", "goals_kept", "free", "reachable", "rounds",
                 "tile_launches", "solve_ms", "max_cost")
    INT_KEYS = ("valid", "dim", "nx", "ny", "nz", "goals", "goals_kept", "free", "reachable", "rounds", "tile_launches")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_plan_create())
        if not self.h:
            raise GpisError("gpis_plan_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_plan_destroy(self.h)
            self.h = None

    __del__ = close

    def set_schedule(self, check_every=0, inner_cap=0):
        """Outer rounds per convergence read-back and relaxation sweeps of a tile per round (0 = defaults 8 / 256; the results
        do not depend on either)."""
        _check(self.L.gpis_plan_set_schedule(self.h, int(check_every), int(inner_cap)), "gpis_plan_set_schedule")

    def solve(self, field, goals, stream=0, **opts):
        """gpis_plan_solve on a DistanceField holding a result; goals [g, dim].  Returns self."""
        inf = field.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        g = np.ascontiguousarray(goals, dtype=np.float32).reshape(-1, inf["dim"])
        o = plan_opts(inf["dim"], inf["step"], **opts)
        _check(self.L.gpis_plan_solve(self.h, field.h, _p(g), g.shape[0], C.byref(o), C.c_void_p(stream)), "gpis_plan_solve")
        return self

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_plan_info(self.h, _p(out, C.c_double), out.size), "gpis_plan_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """(cost f32, policy u8) host copies of the last result, each of shape shape[::-1] (x fastest)."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("planner holds no result")
        shape = (i["nx"], i["ny"], i["nz"])[:i["dim"]][::-1]
        n = int(np.prod(shape))
        cost = np.zeros(n, np.float32)
        pol = np.zeros(n, np.uint8)
        _check(self.L.gpis_plan_get(self.h, _p(cost), _p(pol, C.c_ubyte)), "gpis_plan_get")
        return cost.reshape(shape), pol.reshape(shape)

    def device_ptrs(self):
        """(d_cost, d_policy) device addresses of the last result (0 where there is none)."""
        a, b = C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_plan_device(self.h, C.byref(a), C.byref(b)), "gpis_plan_device")
        return a.value or 0, b.value or 0

    def paths(self, starts, max_points=None, stream=0):
        """Lattice paths from `starts` [m, dim] along the policy (gpis_plan_paths).  Returns (list of [len, dim] float32 arrays,
        start_cost [m], status [m] u8): status 0 arrived, 1 outside / non-finite, 2 not free, 3 unreachable, 4 cut off at
        max_points (default: the number of lattice points, which no path can exceed)."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("planner holds no result")
        dim = i["dim"]
        x = np.ascontiguousarray(starts, dtype=np.float32).reshape(-1, dim)
        if max_points is None:
            max_points = max(2, min(i["nx"] * i["ny"] * i["nz"], 2 ** 31 - 1))
        _check(self.L.gpis_plan_paths(self.h, _p(x), x.shape[0], int(max_points), C.c_void_p(stream)), "gpis_plan_paths")
        m, tot = C.c_longlong(0), C.c_longlong(0)
        _check(self.L.gpis_plan_path_counts(self.h, C.byref(m), C.byref(tot)), "gpis_plan_path_counts")
        off = np.zeros(m.value + 1, np.int64)
        pts = np.zeros((max(tot.value, 1), dim), np.float32)
        sc = np.zeros(m.value, np.float32)
        st = np.zeros(m.value, np.uint8)
        _check(self.L.gpis_plan_get_paths(self.h, _p(off, C.c_longlong), _p(pts), _p(sc), _p(st, C.c_ubyte)), "gpis_plan_get_paths")
        self.last_off = off
        return [pts[off[k]:off[k + 1]] for k in range(m.value)], sc, st

    def trajectories(self, N=64, trajectories=None):
        """The last paths() resampled by arc length to N waypoints each (gpis_traj_from_paths).  Returns the Trajectories
        holding the input (default: a new one), ready for optimize()."""
        t = trajectories if trajectories is not None else Trajectories()
        return t.from_paths(self, N)


def tplan_opts(step, **opts):
    """gpis_tplan_opts of the library's defaults for a field of lattice step `step` (gpis_tplan_default_opts; needs no device)
    with the given fields replaced."""
    o = gpis_tplan_opts()
    _check(lib().gpis_tplan_default_opts(float(step), C.byref(o)), "gpis_tplan_default_opts")
    names = {f[0] for f in gpis_tplan_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown time-plan option %r" % k)
        setattr(o, k, v)
    return o


class _LayeredPlanner:
    """What TimePlanner and TimePosePlanner share: the handle behind gpis_<_PREFIX>_*, info(), the host copies of a result and of
    its paths, the control sequences and follow().  _WHAT names the planner in error messages."""

    _PREFIX = _WHAT = None

    def __init__(self):
        self.L = lib()
        if not hasattr(self.L, "gpis_%s_create" % self._PREFIX):
            raise GpisError("the native library has no %s (gpis_%s_create)" % (self._WHAT, self._PREFIX))
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self._fn("create")())
        if not self.h:
            raise GpisError("gpis_%s_create failed" % self._PREFIX)

    def _fn(self, name):
        return getattr(self.L, "gpis_%s_%s" % (self._PREFIX, name))

    def _call(self, name, *args):
        _check(self._fn(name)(self.h, *args), "gpis_%s_%s" % (self._PREFIX, name))

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    __del__ = close

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        self._call("info", _p(out, C.c_double), out.size)
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def _get(self, dims, cost_all):
        """get() for a layer of the shape given by the info keys `dims`"""
        i = self.info()
        if not i["valid"]:
            raise GpisError("%s holds no result" % self._WHAT)
        shape, S = tuple(i[k] for k in dims), i["horizon"]
        cost0, c = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        pol = np.zeros((S + 1,) + shape, np.uint8)
        call = np.zeros((S + 1,) + shape, np.float32) if cost_all else None
        self._call("get", _p(cost0), _p(pol, C.c_ubyte), _p(call) if cost_all else None, _p(c))
        out = dict(cost0=cost0, policy=pol, c=c)
        if cost_all:
            out["cost_all"] = call
        return out

    def _paths(self, x, stream, heading):
        """paths() from the start rows x; heading: whether the handle's paths carry a heading index per point"""
        self._call("paths", _p(x), x.shape[0], C.c_void_p(stream))
        m, tot = C.c_longlong(0), C.c_longlong(0)
        self._call("path_counts", C.byref(m), C.byref(tot))
        off = np.zeros(m.value + 1, np.int64)
        pts = np.zeros((max(tot.value, 1), 2), np.float32)
        hd = np.zeros(max(tot.value, 1), np.int32)
        arrive = np.zeros(m.value, np.int32)
        sc = np.zeros(m.value, np.float32)
        st = np.zeros(m.value, np.uint8)
        self._call("get_paths", _p(off, C.c_longlong), _p(pts), *([_p(hd, C.c_int)] if heading else []), _p(arrive, C.c_int), _p(sc),
                   _p(st, C.c_ubyte))
        pts, hd = pts[:tot.value], hd[:tot.value]
        out = dict(paths=[pts[off[k]:off[k + 1]] for k in range(m.value)], off=off, points=pts, arrive=arrive, start_cost=sc, status=st)
        if heading:
            out.update(headings=[hd[off[k]:off[k + 1]] for k in range(m.value)], heading=hd)
        return out

    def _npaths(self):
        m = C.c_longlong(0)
        self._call("path_counts", C.byref(m), None)
        return m.value

    def controls(self, T, k0=0, w_limit=0.0, min_move=1e-9):
        """Control sequences of T steps of the plan's slot along the last paths from slot k0 on (gpis_tplan_controls): dict(U
        f64 [m, T, 2], heading0 [m, 2], p0 [m, 2], clamped i32 [m]); a start without a path stands still."""
        m, T = self._npaths(), int(T)
        U = np.zeros((m, max(T, 1), 2), np.float64)
        h0, p0, cl = np.zeros((m, 2), np.float64), np.zeros((m, 2), np.float64), np.zeros(m, np.int32)
        self._call("controls", T, int(k0), float(w_limit), float(min_move), _p(U, C.c_double), _p(h0, C.c_double), _p(p0, C.c_double),
                   _p(cl, C.c_int))
        return dict(U=U, heading0=h0, p0=p0, clamped=cl)

    def follow(self, controller, index, k0=0, w_limit=0.0, min_move=1e-9):
        """Replace `controller`'s nominal sequence by the control sequence of path `index` from slot k0 on, over the controller's
        horizon (controls + gpis_mppi_set_nominal; the controller is meant to run at dt = the plan's slot).  Returns (p0 [2],
        heading0 [2])."""
        i = controller.info()
        if not i["inited"] or i["dim"] != 2:
            raise GpisError("follow needs a 2-D controller after init")
        r = self.controls(i["horizon"], k0, w_limit, min_move)
        controller.set_nominal(r["U"][int(index)])
        return r["p0"][int(index)].copy(), r["heading0"][int(index)].copy()


class TimePlanner(_LayeredPlanner):
    """Result holder of the planner through space and time (gpis_tplan_*): a policy byte per (lattice point, slot), the cost of
    slot 0, paths, their check against moving balls and their control sequences, on the device; buffers reused across calls.
    A finished plan depends neither on the field nor on the set it was solved with."""

    INFO_KEYS = ("valid", "nx", "ny", "horizon", "slot", "balls", "goals", "goals_kept", "free", "finite0", "layer_launches",
                 "skipped", "solve_ms", "max_cost0", "t_begin", "keep_cost")
    INT_KEYS = ("valid", "nx", "ny", "horizon", "balls", "goals", "goals_kept", "free", "finite0", "layer_launches", "skipped",
                "keep_cost")

    _PREFIX, _WHAT = "tplan", "time planner"

    def set_schedule(self, layers_per_launch=0, cull=1):
        """Layers a launch advances (0 = the default: 4 without balls, 1 with them; at most 16) and the broad phase over the balls (0 / 1); the results do not
        depend on either."""
        _check(self.L.gpis_tplan_set_schedule(self.h, int(layers_per_launch), int(cull)), "gpis_tplan_set_schedule")
        return self

    def solve(self, field, goals, obstacles=None, t_begin=0.0, stream=0, **opts):
        """gpis_tplan_solve on a 2-D DistanceField holding a result; goals [g, 2]; obstacles: an Obstacles or None.  Returns
        self."""
        inf = field.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        g = np.ascontiguousarray(goals, dtype=np.float32).reshape(-1, 2)
        o = tplan_opts(inf["step"], **opts)
        _check(self.L.gpis_tplan_solve(self.h, field.h, obstacles.h if obstacles is not None else None, _p(g), g.shape[0],
                                       float(t_begin), C.byref(o), C.c_void_p(stream)), "gpis_tplan_solve")
        self.dyn_clearance = float(o.dyn_clearance)
        return self

    def get(self, cost_all=False):
        """dict(cost0 f32 [ny, nx], policy u8 [S + 1, ny, nx], c f32 [ny, nx]) host copies of the last result, with cost_all
        f32 [S + 1, ny, nx] on request (the solve must have kept it)."""
        return self._get(("ny", "nx"), cost_all)

    def device_ptrs(self):
        """(d_cost0, d_policy) device addresses of the last result (0 where there is none)."""
        a, b = C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_tplan_device(self.h, C.byref(a), C.byref(b)), "gpis_tplan_device")
        return a.value or 0, b.value or 0

    def paths(self, starts, stream=0):
        """Routes from `starts` [m, 2] at slot 0 along the policy (gpis_tplan_paths).  Returns dict(paths: list of [arrive + 1,
        2] float32 arrays, one point per slot; off i64 [m + 1]; points f32 [total, 2]; arrive i32 [m]; start_cost f32 [m];
        status u8 [m]: 0 arrived, 1 outside / non-finite, 2 not free, 3 no arrival within the horizon)."""
        return self._paths(np.ascontiguousarray(starts, dtype=np.float32).reshape(-1, 2), stream, False)

    def check(self, obstacles, clearance=None):
        """The last paths against the balls of `obstacles` (any 2-D set: the solve's, or a newer detection) at the solve's
        t_begin and slot (gpis_tplan_check): dict(min_sep, min_time f64 [m], min_obstacle, first_hit, collides i32 [m]).
        clearance None: the last solve's dyn_clearance."""
        m = self._npaths()
        if clearance is None:
            clearance = self.dyn_clearance
        ms, mt = np.zeros(m, np.float64), np.zeros(m, np.float64)
        mo, fh, co = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        _check(self.L.gpis_tplan_check(self.h, obstacles.h, float(clearance), _p(ms, C.c_double), _p(mt, C.c_double), _p(mo, C.c_int),
                                       _p(fh, C.c_int), _p(co, C.c_int)), "gpis_tplan_check")
        return dict(min_sep=ms, min_time=mt, min_obstacle=mo, first_hit=fh, collides=co)


POSE_HEADINGS = (8, 16, 32, 64)
# the direction of translation code k as a multiple of 45 degrees anticlockwise from +x
_POSE_ANGLE8 = {14: 0, 17: 1, 16: 2, 15: 3, 12: 4, 9: 5, 10: 6, 11: 7}


def pplan_opts(step, H=16, **opts):
    """gpis_pplan_opts of the library's defaults for a field of lattice step `step` and H headings (gpis_pplan_default_opts)
    with the given fields replaced."""
    o = gpis_pplan_opts()
    _check(lib().gpis_pplan_default_opts(float(step), int(H), C.byref(o)), "gpis_pplan_default_opts")
    names = {f[0] for f in gpis_pplan_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown pose plan option %r" % k)
        setattr(o, k, v)
    return o


def heading_table(H):
    """[H, 2] float64 (cos, sin) of 2 pi h / H with exact 0 / +-1 at the quarter turns: the table PosePlanner.solve takes."""
    H = int(H)
    if H not in POSE_HEADINGS:
        raise GpisError("H must be one of 8, 16, 32, 64")
    t = np.zeros((H, 2), np.float64)
    q = H // 4
    exact = {0: (1.0, 0.0), q: (0.0, 1.0), 2 * q: (-1.0, 0.0), 3 * q: (0.0, -1.0)}
    for h in range(H):
        t[h] = exact[h] if h in exact else (math.cos(2.0 * math.pi * h / H), math.sin(2.0 * math.pi * h / H))
    return t


def heading_moves(H, mode="any"):
    """uint16 [H]: bit k - 9 set iff the translation of direction code k is allowed at heading index h.  The direction of code
    k has the heading index a_k H / 8.  "any": all 8 directions; "forward": those within H / 16 heading steps of h
    (16 circdist(h, a_k H / 8) <= H); "both": those or their opposites.  Integers only."""
    H = int(H)
    if H not in POSE_HEADINGS:
        raise GpisError("H must be one of 8, 16, 32, 64")
    if mode not in ("any", "forward", "both"):
        raise GpisError("mode must be any, forward or both")
    out = np.zeros(H, np.uint16)
    for h in range(H):
        for k, a in _POSE_ANGLE8.items():
            ok = mode == "any"
            for aa in ((a,) if mode == "forward" else (a, (a + 4) % 8)):
                d = abs(h - aa * H // 8) % H
                ok = ok or 16 * min(d, H - d) <= H
            if ok:
                out[h] |= np.uint16(1 << (k - 9))
    return out


def _pose_rows(a):
    """float32 [n, 3] = (x, y, h) rows of a [n, 3], [n, 2], [3] or [2] array; rows without a heading get h = -1."""
    a = np.asarray(a, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a.reshape(a.shape[0], -1)
    if a.shape[1] == 2:
        a = np.concatenate([a, np.full((a.shape[0], 1), -1, np.float32)], axis=1)
    if a.shape[1] != 3:
        raise GpisError("poses must have 2 or 3 columns")
    return np.ascontiguousarray(a, dtype=np.float32)


class PosePlanner:
    """Result holder of the pose planner (gpis_pplan_*): cost-to-go and policy over poses (x, y, heading) of a 2-D field for a
    Footprint, pose paths, and the projection into a Planner.  A finished plan depends neither on the field nor on the
    footprint it was solved with."""

    INFO_KEYS = ("valid", "nx", "ny", "H", "step", "goals", "goals_kept", "free", "reachable", "rounds", "tile_launches", "solve_ms",
                 "max_cost", "setup_ms")
    INT_KEYS = ("valid", "nx", "ny", "H", "goals", "goals_kept", "free", "reachable", "rounds", "tile_launches")

    def __init__(self):
        self.L = lib()
        if not hasattr(self.L, "gpis_pplan_create"):
            raise GpisError("the native library has no pose planner (gpis_pplan_create)")
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_pplan_create())
        if not self.h:
            raise GpisError("gpis_pplan_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_pplan_destroy(self.h)
            self.h = None

    __del__ = close

    def set_schedule(self, check_every=0, inner_cap=0):
        """Outer rounds per convergence read-back and relaxation sweeps of a tile per round (0 = defaults 8 / 256; the results
        do not depend on either)."""
        _check(self.L.gpis_pplan_set_schedule(self.h, int(check_every), int(inner_cap)), "gpis_pplan_set_schedule")

    def solve(self, field, footprint, goals, H=16, moves="any", headings=None, stream=0, **opts):
        """gpis_pplan_solve on a 2-D DistanceField holding a result for a Footprint; goals [g, 3] = (x, y, h), h = -1 meaning
        every free heading (goals [g, 2] are taken as that).  moves: a mode of heading_moves or a uint16 [H] table; headings:
        a [H, 2] table (default heading_table(H)).  opts: the gpis_pplan_opts fields.  Returns self."""
        inf = field.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        H = int(H)
        g = _pose_rows(goals)
        tab = np.ascontiguousarray(heading_table(H) if headings is None else headings, dtype=np.float64).reshape(-1, 2)
        mv = np.ascontiguousarray(heading_moves(H, moves) if isinstance(moves, str) else moves, dtype=np.uint16).ravel()
        if tab.shape[0] != H or mv.size != H:
            raise GpisError("headings and moves must have H rows")
        o = pplan_opts(inf["step"], H, **opts)
        _check(self.L.gpis_pplan_solve(self.h, field.h, footprint.h, _p(tab, C.c_double), _p(mv, C.c_ushort), H, _p(g), g.shape[0],
                                       C.byref(o), C.c_void_p(stream)), "gpis_pplan_solve")
        return self

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_pplan_info(self.h, _p(out, C.c_double), out.size), "gpis_pplan_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """(cost f32, policy u8, c f32) host copies of the last result, each of shape (H, ny, nx)."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("pose planner holds no result")
        shape = (i["H"], i["ny"], i["nx"])
        n = int(np.prod(shape))
        cost, pol, c = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
        _check(self.L.gpis_pplan_get(self.h, _p(cost), _p(pol, C.c_ubyte), _p(c)), "gpis_pplan_get")
        return cost.reshape(shape), pol.reshape(shape), c.reshape(shape)

    def device_ptrs(self):
        """(d_cost, d_policy, d_c) device addresses of the last result (0 where there is none)."""
        a, b, c = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_pplan_device(self.h, C.byref(a), C.byref(b), C.byref(c)), "gpis_pplan_device")
        return a.value or 0, b.value or 0, c.value or 0

    def paths(self, starts, max_points=None, stream=0):
        """Pose paths from `starts` [m, 3] = (x, y, h) along the policy (gpis_pplan_paths); h = -1: the free heading of least
        cost there ([m, 2] starts are taken as that).  Returns (list of [len, 2] float32 points, list of [len] int32 heading
        indices, start_cost [m], status [m] u8) with gpis_plan_paths' status codes; max_points defaults to the number of
        states, which no path can exceed."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("pose planner holds no result")
        x = _pose_rows(starts)
        if max_points is None:
            max_points = max(2, min(i["nx"] * i["ny"] * i["H"], 2 ** 31 - 1))
        _check(self.L.gpis_pplan_paths(self.h, _p(x), x.shape[0], int(max_points), C.c_void_p(stream)), "gpis_pplan_paths")
        m, tot = C.c_longlong(0), C.c_longlong(0)
        _check(self.L.gpis_pplan_path_counts(self.h, C.byref(m), C.byref(tot)), "gpis_pplan_path_counts")
        off = np.zeros(m.value + 1, np.int64)
        pts = np.zeros((max(tot.value, 1), 2), np.float32)
        hd = np.zeros(max(tot.value, 1), np.int32)
        sc = np.zeros(m.value, np.float32)
        st = np.zeros(m.value, np.uint8)
        _check(self.L.gpis_pplan_get_paths(self.h, _p(off, C.c_longlong), _p(pts), _p(hd, C.c_int), _p(sc), _p(st, C.c_ubyte)),
               "gpis_pplan_get_paths")
        self.last_off = off
        return ([pts[off[k]:off[k + 1]] for k in range(m.value)], [hd[off[k]:off[k + 1]] for k in range(m.value)], sc, st)

    def trajectories(self, N=64, trajectories=None):
        """The points of the last paths() resampled by arc length to N waypoints each (gpis_smooth_from_pose_paths; the heading
        indices are not carried over).  Returns the Trajectories holding the input (default: a new one), ready for
        optimize(field, footprint=...)."""
        t = trajectories if trajectories is not None else Trajectories()
        return t.from_pose_paths(self, N)

    def project(self, planner=None):
        """The 2-D summary of the last result in a Planner (gpis_pplan_project; default: a new one): cost2 = the least cost
        over the headings, a policy that descends it, c2 = the least point cost over the free headings.  Planner.paths,
        Planner.trajectories and Controller.step(planner=...) take it as any solved Planner.  self.heading2 [ny, nx] u8 is the
        first heading attaining cost2 (255: none).  The projection is a guide; the pose path is the certificate."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("pose planner holds no result")
        p = planner if planner is not None else Planner()
        h2 = np.zeros(i["nx"] * i["ny"], np.uint8)
        _check(self.L.gpis_pplan_project(self.h, p.h, _p(h2, C.c_ubyte)), "gpis_pplan_project")
        self.heading2 = h2.reshape(i["ny"], i["nx"])
        return p


def tpplan_opts(step, H=16, **opts):
    """gpis_tpplan_opts of the library's defaults for a field of lattice step `step` and H headings (gpis_tpplan_default_opts;
    needs no device) with the given fields replaced."""
    o = gpis_tpplan_opts()
    _check(lib().gpis_tpplan_default_opts(float(step), int(H), C.byref(o)), "gpis_tpplan_default_opts")
    names = {f[0] for f in gpis_tpplan_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown time-pose-plan option %r" % k)
        setattr(o, k, v)
    return o


class TimePosePlanner(_LayeredPlanner):
    """Result holder of the time-pose planner (gpis_tpplan_*): a policy byte per (lattice point, heading index, slot), the cost
    of slot 0, pose paths, their check against moving balls with a footprint, and their control sequences, on the device;
    buffers reused across calls.  A finished plan depends on neither the field, the set nor the footprint it was solved with."""

    INFO_KEYS = ("valid", "nx", "ny", "H", "horizon", "slot", "balls", "body_balls", "goals", "goals_kept", "free", "finite0",
                 "max_cost0", "t_begin", "keep_cost", "launches", "skipped", "solve_ms")
    INT_KEYS = ("valid", "nx", "ny", "H", "horizon", "balls", "body_balls", "goals", "goals_kept", "free", "finite0", "keep_cost",
                "launches", "skipped")

    _PREFIX, _WHAT = "tpplan", "time-pose planner"

    def set_schedule(self, cull=1):
        """The broad phase over the balls (0 / 1); the results do not depend on it."""
        _check(self.L.gpis_tpplan_set_schedule(self.h, int(cull)), "gpis_tpplan_set_schedule")
        return self

    def solve(self, field, goals, footprint, obstacles=None, H=16, moves="any", t_begin=0.0, headings=None, stream=0, **opts):
        """gpis_tpplan_solve on a 2-D DistanceField holding a result for a Footprint; goals [g, 3] = (x, y, h), h = -1 meaning
        every free heading (goals [g, 2] are taken as that); obstacles: an Obstacles or None.  moves: a mode of heading_moves
        or a uint16 [H] table; headings: a [H, 2] table (default heading_table(H)).  Returns self."""
        inf = field.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        H = int(H)
        g = _pose_rows(goals)
        tab = np.ascontiguousarray(heading_table(H) if headings is None else headings, dtype=np.float64).reshape(-1, 2)
        mv = np.ascontiguousarray(heading_moves(H, moves) if isinstance(moves, str) else moves, dtype=np.uint16).ravel()
        if tab.shape[0] != H or mv.size != H:
            raise GpisError("headings and moves must have H rows")
        o = tpplan_opts(inf["step"], H, **opts)
        _check(self.L.gpis_tpplan_solve(self.h, field.h, obstacles.h if obstacles is not None else None, footprint.h,
                                        _p(tab, C.c_double), _p(mv, C.c_ushort), H, _p(g), g.shape[0], float(t_begin), C.byref(o),
                                        C.c_void_p(stream)), "gpis_tpplan_solve")
        self.dyn_clearance = float(o.dyn_clearance)
        return self

    def get(self, cost_all=False):
        """dict(cost0 f32 [H, ny, nx], policy u8 [S + 1, H, ny, nx], c f32 [H, ny, nx]) host copies of the last result, with
        cost_all f32 [S + 1, H, ny, nx] on request (the solve must have kept it)."""
        return self._get(("H", "ny", "nx"), cost_all)

    def paths(self, starts, stream=0):
        """Pose routes from `starts` [m, 3] = (x, y, h) at slot 0 along the policy (gpis_tpplan_paths); h = -1: the free heading
        of least cost there ([m, 2] starts are taken as that).  Returns dict(paths: list of [arrive + 1, 2] float32 points, one
        per slot; headings: list of [arrive + 1] int32 heading indices; off i64 [m + 1]; points f32 [total, 2]; heading i32
        [total]; arrive i32 [m]; start_cost f32 [m]; status u8 [m]: 0 arrived, 1 outside / non-finite, 2 not free, 3 no arrival
        within the horizon)."""
        return self._paths(_pose_rows(starts), stream, True)

    def check(self, obstacles, footprint=None, clearance=None):
        """The last paths against the balls of `obstacles` (any 2-D set) with `footprint` (any 2-D Footprint; None: the solve's)
        at the solve's t_begin, slot and heading table (gpis_tpplan_check): dict(min_sep, min_time f64 [m], min_obstacle,
        min_ball, first_hit, collides i32 [m]).  clearance None: the last solve's dyn_clearance."""
        m = self._npaths()
        if clearance is None:
            clearance = self.dyn_clearance
        ms, mt = np.zeros(m, np.float64), np.zeros(m, np.float64)
        mo, mb, fh, co = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        _check(self.L.gpis_tpplan_check(self.h, obstacles.h, footprint.h if footprint is not None else None, float(clearance),
                                        _p(ms, C.c_double), _p(mt, C.c_double), _p(mo, C.c_int), _p(mb, C.c_int), _p(fh, C.c_int),
                                        _p(co, C.c_int)), "gpis_tpplan_check")
        return dict(min_sep=ms, min_time=mt, min_obstacle=mo, min_ball=mb, first_hit=fh, collides=co)

    def controls(self, T, k0=0, w_limit=0.0, min_move=1e-9):
        """Control sequences of T steps of the plan's slot along the points of the last paths from slot k0 on
        (gpis_tpplan_controls): dict(U f64 [m, T, 2], heading0 [m, 2], p0 [m, 2], clamped i32 [m]); a start without a path
        stands still.  The heading indices are not tracked: the pose path is the certificate, the controls are a guide."""
        return super().controls(T, k0, w_limit, min_move)


def cover_opts(dim, step, **opts):
    """gpis_cover_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_cover_default_opts) with the
    given fields replaced."""
    o = gpis_cover_opts()
    _check(lib().gpis_cover_default_opts(int(dim), float(step), C.byref(o)), "gpis_cover_default_opts")
    names = {f[0] for f in gpis_cover_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown coverage option %r" % k)
        setattr(o, k, v)
    return o


class Coverage:
    """Which lattice points of a field a sensor has seen as free space (gpis_cover_*): one byte per point on the device, the
    frontiers of the seen space, and fields restricted to it.  reset(field) takes the field's lattice; every later call wants a
    field of that lattice."""

    INFO_KEYS = ("valid", "dim", "nx", "ny", "nz", "step", "frames", "frontiers", "points", "components", "clusters", "rounds",
                 "integrate_ms", "frontiers_ms")
    INT_KEYS = ("valid", "dim", "nx", "ny", "nz", "frames", "frontiers", "points", "components", "clusters", "rounds")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_cover_create())
        if not self.h:
            raise GpisError("gpis_cover_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_cover_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self, field):
        """The lattice of `field` (a DistanceField holding a result), nothing seen.  Returns self."""
        _check(self.L.gpis_cover_reset(self.h, field.h), "gpis_cover_reset")
        return self

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_cover_info(self.h, _p(out, C.c_double), out.size), "gpis_cover_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def _lattice(self):
        i = self.info()
        if not i["valid"]:
            raise GpisError("coverage holds no lattice: reset(field) first")
        return i, (i["nx"], i["ny"], i["nz"])[:i["dim"]]

    def _opts(self, opts):
        i, _ = self._lattice()
        return cover_opts(i["dim"], i["step"], **opts)

    def integrate_depth(self, depth, pose, cam6, map=None, stream=None, **opts):
        """Mark what a depth frame sees as free space (gpis3_cover_depth): a lattice point is seen iff it projects into the
        image, its nearest pixel's depth is valid and the point lies more than back_off in front of it.  depth [W*H]
        column-major as update(); pose [12] f32; cam6 None: the camera of `map` (a GPisMap3).  opts: back_off.  Returns self."""
        return self._integrate_depth(map.h if map is not None else None, map._wh if map is not None else None,
                                     depth, pose, cam6, stream, opts)

    def integrate_scan(self, thetas, ranges, pose6, off2, map=None, stream=None, **opts):
        """Mark what a laser scan sees as free space (gpis2_cover_scan): a lattice point is seen iff it lies between two
        neighbouring valid beams no more than max_gap apart and closer than the nearer of their ranges less back_off.  off2
        None: the sensor offset of `map` (a GPisMap).  opts: back_off, max_gap.  Returns self."""
        return self._integrate_scan(map.h if map is not None else None, thetas, ranges, pose6, off2, stream, opts)

    def _integrate_depth(self, map_h, map_wh, depth, pose, cam6, stream, opts):
        pose = np.ascontiguousarray(pose, dtype=np.float32).ravel()
        if pose.size != 12:
            raise GpisError("pose must have 12 elements")
        depth, cam = _depth_frame("integrate_depth", depth, cam6, map_h, map_wh)
        o = self._opts(opts)
        _check(self.L.gpis3_cover_depth(map_h, self.h, cam, _p(depth), _p(pose), C.byref(o), C.c_void_p(stream or 0)),
               "gpis3_cover_depth")
        return self

    def _integrate_scan(self, map_h, thetas, ranges, pose6, off2, stream, opts):
        pose6 = np.ascontiguousarray(pose6, dtype=np.float32).ravel()
        if pose6.size != 6:
            raise GpisError("pose6 must have 6 elements")
        thetas, ranges, off = _scan_frame("integrate_scan", thetas, ranges, off2, map_h)
        o = self._opts(opts)
        _check(self.L.gpis2_cover_scan(map_h, self.h, _p(thetas), _p(ranges), thetas.size, _p(pose6), off, C.byref(o),
                                       C.c_void_p(stream or 0)), "gpis2_cover_scan")
        return self

    def set(self, seen):
        """Upload the mask (any array of the lattice's point count, x fastest; non-zero = seen).  Returns self."""
        _, shape = self._lattice()
        m = np.ascontiguousarray(np.asarray(seen) != 0, dtype=np.uint8).ravel()
        if m.size != int(np.prod(shape)):
            raise GpisError("the mask must have %d elements" % int(np.prod(shape)))
        _check(self.L.gpis_cover_set(self.h, _p(m, C.c_ubyte), m.size), "gpis_cover_set")
        return self

    def get(self):
        """The mask, uint8 of shape shape[::-1] (x fastest)."""
        _, shape = self._lattice()
        m = np.zeros(int(np.prod(shape)), np.uint8)
        _check(self.L.gpis_cover_get(self.h, _p(m, C.c_ubyte), m.size), "gpis_cover_get")
        return m.reshape(shape[::-1])

    def device_ptr(self):
        """Device address of the mask (0 before reset)."""
        a = C.c_void_p(0)
        _check(self.L.gpis_cover_device(self.h, C.byref(a)), "gpis_cover_device")
        return a.value or 0

    def frontiers(self, field, points=False, stream=None, **opts):
        """The frontiers of the seen space on `field` (gpis_cover_frontiers): seen points with dist >= clearance that have an
        unseen axis neighbour with dist >= clearance, clustered under full connectivity.  opts: clearance, min_size,
        max_rounds.  Returns a dict over the clusters of at least min_size points, ordered by label: label (the smallest
        lattice index), count, centroid [c, dim] (world, double), rep [c, dim] (float32: the member lattice point nearest the
        centroid), rep_index, sums [c, 3], box [c, 6] (min i, j, k, max i, j, k), and npoints / ncomponents; with points=True
        also points [m] (ascending lattice indices) and point_label [m]."""
        i, shape = self._lattice()
        dim = i["dim"]
        o = self._opts(opts)
        _check(self.L.gpis_cover_frontiers(self.h, field.h, C.byref(o), C.c_void_p(stream or 0)), "gpis_cover_frontiers")
        m, nc, c = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(self.L.gpis_cover_counts(self.h, C.byref(m), C.byref(nc), C.byref(c)), "gpis_cover_counts")
        m, nc, c = m.value, nc.value, c.value
        label, count, rep = np.zeros(c, np.int32), np.zeros(c, np.int32), np.zeros(c, np.int32)
        sums, box = np.zeros((c, 3), np.int64), np.zeros((c, 6), np.int32)
        pts = np.zeros(m, np.int32) if points else None
        pl = np.zeros(m, np.int32) if points else None
        _check(self.L.gpis_cover_get_frontiers(self.h, _p(label, C.c_int), _p(count, C.c_int), _p(sums, C.c_longlong), _p(box, C.c_int),
                                               _p(rep, C.c_int), _p(pts, C.c_int) if points else None,
                                               _p(pl, C.c_int) if points else None), "gpis_cover_get_frontiers")
        finf = field.info()
        o32 = np.asarray(finf["origin"], np.float32)
        st = np.float32(finf["step"])
        nx, ny = shape[0], shape[1]
        r64 = rep.astype(np.int64)
        ijk = np.stack([r64 % nx, (r64 // nx) % ny, r64 // (nx * ny)], axis=1)[:, :dim]
        out = dict(label=label, count=count, sums=sums, box=box, rep_index=rep, npoints=m, ncomponents=nc,
                   rep=(o32[None, :] + ijk.astype(np.float32) * st).astype(np.float32).reshape(c, dim),
                   centroid=o32.astype(np.float64)[None, :] + (sums[:, :dim].astype(np.float64)
                                                               / np.maximum(count, 1).astype(np.float64)[:, None]) * np.float64(st))
        if points:
            out["points"], out["point_label"] = pts, pl
        return out

    def restrict(self, field, out=None, unseen_dist=None, stream=None):
        """A copy of `field` restricted to seen space (gpis_cover_restrict): dist = seen ? field's : unseen_dist (default -step:
        blocked at any clearance >= 0, and finite for the sampler).  out: the DistanceField to fill (default: one kept by this
        coverage; never `field` itself).  Returns it: everything that takes a DistanceField runs on it unchanged."""
        if out is None:
            if getattr(self, "_restricted", None) is None:
                self._restricted = DistanceField()
            out = self._restricted
        u = -field._step() if unseen_dist is None else float(unseen_dist)
        _check(self.L.gpis_cover_restrict(self.h, field.h, out.h, u, C.c_void_p(stream or 0)), "gpis_cover_restrict")
        out._device = field.device()
        return out


def detect_opts(dim, step, **opts):
    """gpis_detect_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_detect_default_opts) with
    the given fields replaced."""
    o = gpis_detect_opts()
    _check(lib().gpis_detect_default_opts(int(dim), float(step), C.byref(o)), "gpis_detect_default_opts")
    names = {f[0] for f in gpis_detect_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown detector option %r" % k)
        setattr(o, k, v)
    return o


class Detector:
    """Moving obstacles from a frame's residual against a field (gpis_detect_*): holds the device result of the last
    DistanceField.detect_scan / detect_depth call and the tracks that give the balls their ids, ages and velocities."""

    INFO_KEYS = ("valid", "dim", "grid", "grid_w", "grid_h", "samples", "foreign", "components", "balls", "noise", "too_large",
                 "dropped", "rounds", "tracks", "tracks_held", "t_prev", "ms", "setup_ms", "flag_ms", "compact_ms", "label_ms",
                 "table_ms")
    INT_KEYS = INFO_KEYS[:15]

    def __init__(self):
        self.L = lib()
        if not hasattr(self.L, "gpis_detect_create"):
            raise GpisError("the native library has no detector (gpis_detect_create)")
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_detect_create())
        if not self.h:
            raise GpisError("gpis_detect_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_detect_destroy(self.h)
            self.h = None

    __del__ = close

    def set_schedule(self, check_every=0, profile=False):
        """Labelling rounds per read-back (1 .. 64; 0 keeps it) and whether every stage is synchronised for its time."""
        _check(self.L.gpis_detect_set_schedule(self.h, int(check_every), int(bool(profile))), "gpis_detect_set_schedule")
        return self

    def reset_tracks(self):
        _check(self.L.gpis_detect_reset_tracks(self.h), "gpis_detect_reset_tracks")
        return self

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_detect_info(self.h, _p(out, C.c_double), out.size), "gpis_detect_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def _counts(self):
        g, c, b = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _check(self.L.gpis_detect_counts(self.h, C.byref(g), C.byref(c), C.byref(b)), "gpis_detect_counts")
        return g.value, c.value, b.value

    def result(self):
        """The balls of the last call: dict(centre, velocity [b, dim] f64, radius [b] f64, count, label, id, age, missed [b]
        i32, box [b, 2, dim] f32 (least, greatest), and the counts samples, foreign, components, noise, too_large, dropped,
        rounds).  Detected balls come in label order; coasting ones (count 0, label -1) follow in id order."""
        i = self.info()
        _, _, b = self._counts()
        dim = i["dim"]
        c, v, r = np.zeros((b, dim), np.float64), np.zeros((b, dim), np.float64), np.zeros(b, np.float64)
        cnt, lab, ids, age, mis = (np.zeros(b, np.int32) for _ in range(5))
        box = np.zeros((b, 6), np.float32)
        _check(self.L.gpis_detect_get_balls(self.h, _p(c, C.c_double), _p(v, C.c_double), _p(r, C.c_double), _p(cnt, C.c_int), _p(box),
                                            _p(lab, C.c_int), _p(ids, C.c_int), _p(age, C.c_int), _p(mis, C.c_int)),
               "gpis_detect_get_balls")
        out = dict(centre=c, velocity=v, radius=r, count=cnt, label=lab, id=ids, age=age, missed=mis,
                   box=np.ascontiguousarray(box.reshape(b, 2, 3)[:, :, :dim]))
        for k in ("samples", "foreign", "components", "noise", "too_large", "dropped", "rounds"):
            out[k] = i[k]
        return out

    def components(self):
        """Every component of the last call in label order: dict(label, count, flag [c] i32 (0 ball, 1 noise, 2 too large, 3
        dropped for the cap), box [c, 2, dim] f32, centre [c, dim] f64, r2 [c] f64)."""
        _, nc, _ = self._counts()
        dim = self.info()["dim"]
        lab, cnt, flg = np.zeros(nc, np.int32), np.zeros(nc, np.int32), np.zeros(nc, np.int32)
        box, ctr, r2 = np.zeros((nc, 6), np.float32), np.zeros((nc, 3), np.float64), np.zeros(nc, np.float64)
        _check(self.L.gpis_detect_get_components(self.h, _p(lab, C.c_int), _p(cnt, C.c_int), _p(box), _p(ctr, C.c_double),
                                                 _p(r2, C.c_double), _p(flg, C.c_int)), "gpis_detect_get_components")
        return dict(label=lab, count=cnt, flag=flg, box=np.ascontiguousarray(box.reshape(nc, 2, 3)[:, :, :dim]),
                    centre=np.ascontiguousarray(ctr[:, :dim]), r2=r2)

    def samples(self):
        """Per sample of the grid (the beams; 3-D: the W // stride x H // stride strided pixels, column-major): dict(label i32
        (the component's smallest grid index; -1: not foreign or not valid), d f32 (NaN: not valid, or off the lattice), x
        [g, dim] f32, foreign u8)."""
        g, _, _ = self._counts()
        dim = self.info()["dim"]
        lab, d, x, f = np.full(g, -1, np.int32), np.full(g, np.nan, np.float32), np.zeros((g, dim), np.float32), np.zeros(g, np.uint8)
        _check(self.L.gpis_detect_get_samples(self.h, _p(lab, C.c_int), _p(d), _p(x), _p(f, C.c_ubyte)), "gpis_detect_get_samples")
        return dict(label=lab, d=d, x=x, foreign=f)

    def to_obstacles(self, obstacles):
        """Hand the current balls to an Obstacles set (gpis_detect_to_obstacles): centres, velocities and radii with epoch =
        the call's t; the set's cost options stay; no balls empties the set.  Returns the set."""
        _check(self.L.gpis_detect_to_obstacles(self.h, obstacles.h), "gpis_detect_to_obstacles")
        return obstacles


def view_opts(dim, step, **opts):
    """gpis_view_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_view_default_opts) with the
    given fields replaced; the fields of the march (gpis_render_field_opts) are taken by name as well."""
    o = gpis_view_opts()
    _check(lib().gpis_view_default_opts(int(dim), float(step), C.byref(o)), "gpis_view_default_opts")
    own = {f[0] for f in gpis_view_opts._fields_} - {"march"}
    march = {f[0] for f in gpis_render_field_opts._fields_}
    for k, v in opts.items():
        if k in own:
            setattr(o, k, v)
        elif k in march:
            setattr(o.march, k, v)
        else:
            raise GpisError("unknown view option %r" % k)
    return o


class ViewScorer:
    """Holds the device buffers and the last result of a batch of candidate viewpoints scored against a field and a coverage
    (gpis*_view_gain_*): per pose the number of unseen lattice points it would reveal and the rays with a predicted return."""

    INFO_KEYS = ("valid", "dim", "poses", "rays", "targets", "samples", "predict_ms", "table_ms", "target_ms", "gather_ms")
    INT_KEYS = ("valid", "dim", "poses", "rays", "targets", "samples")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_view_create())
        if not self.h:
            raise GpisError("gpis_view_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_view_destroy(self.h)
            self.h = None

    __del__ = close

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_view_info(self.h, _p(out, C.c_double), out.size), "gpis_view_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """(gain int64 [m], hits int32 [m]) of the last call."""
        m = self.info()["poses"]
        gain, hits = np.zeros(m, np.int64), np.zeros(m, np.int32)
        _check(self.L.gpis_view_get(self.h, _p(gain, C.c_longlong), _p(hits, C.c_int), m), "gpis_view_get")
        return gain, hits

    def gain(self):
        return self.get()[0]

    def hits(self):
        return self.get()[1]

    def predicted(self, k):
        """The predicted measurement d' [rays] f32 of pose k of the last call (3-D: column-major as update())."""
        out = np.zeros(self.info()["rays"], np.float32)
        _check(self.L.gpis_view_get_predicted(self.h, int(k), _p(out), out.size), "gpis_view_get_predicted")
        return out


def traj_opts(dim, step, **opts):
    """gpis_traj_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_traj_default_opts) with the
    given fields replaced."""
    o = gpis_traj_opts()
    _check(lib().gpis_traj_default_opts(int(dim), float(step), C.byref(o)), "gpis_traj_default_opts")
    names = {f[0] for f in gpis_traj_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown trajectory option %r" % k)
        setattr(o, k, v)
    return o


def traj_body_opts(dim, step, balls, **opts):
    """(gpis_traj_opts, w_turn) of the library's defaults for smoothing with a footprint of `balls` balls
    (gpis_smooth_body_default_opts: traj_opts with w_obs = 0.25 step / balls; w_turn = 1) with the given fields replaced."""
    o, wt = gpis_traj_opts(), C.c_float(0)
    _check(lib().gpis_smooth_body_default_opts(int(dim), float(step), int(balls), C.byref(o), C.byref(wt)), "gpis_smooth_body_default_opts")
    names = {f[0] for f in gpis_traj_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown trajectory option %r" % k)
        setattr(o, k, v)
    return o, float(wt.value)


class Trajectories:
    """Input and result holder of the trajectory optimiser (gpis_traj_*): a batch of m trajectories of N waypoints on the
    device, buffers reused across calls.  optimize() always starts from the input; a result does not depend on the field or the
    planner it came from."""

    INFO_KEYS = ("input", "valid", "m", "N", "dim", "ms")
    INT_KEYS = ("input", "valid", "m", "N", "dim")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_traj_create())
        if not self.h:
            raise GpisError("gpis_traj_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_traj_destroy(self.h)
            self.h = None

    __del__ = close

    def from_paths(self, planner, N=64):
        """The input from the planner's last paths() resampled by arc length to N waypoints each (gpis_traj_from_paths); a
        path of another status than 0 gives a trajectory of status 2.  Returns self."""
        _check(self.L.gpis_traj_from_paths(self.h, planner.h, int(N)), "gpis_traj_from_paths")
        return self

    def set(self, x):
        """The input from waypoints x [m, N, dim] (gpis_traj_set).  Returns self."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 3:
            raise GpisError("waypoints must be [m, N, dim]")
        _check(self.L.gpis_traj_set(self.h, _p(x), x.shape[0], x.shape[1], x.shape[2]), "gpis_traj_set")
        return self

    def from_pose_paths(self, pose_planner, N=64):
        """The input from the points of a PosePlanner's last paths() resampled as from_paths does (gpis_smooth_from_pose_paths); a
        turn in place repeats a point and takes no part of the length.  Returns self."""
        _check(self.L.gpis_smooth_from_pose_paths(self.h, pose_planner.h, int(N)), "gpis_smooth_from_pose_paths")
        return self

    def optimize(self, field, footprint=None, w_turn=None, stream=0, **opts):
        """gpis_traj_optimize on a DistanceField holding a result.  footprint: a Footprint whose balls take the obstacle term in
        the waypoint's place, the body facing along its chord (gpis_smooth_body_optimize; the defaults are traj_body_opts');
        w_turn weighs the term that turns the chords (default 1).  Returns self."""
        inf = field.info()
        if inf["dim"] == 0:
            raise GpisError("distance field holds no result")
        if footprint is None:
            if w_turn is not None:
                raise GpisError("w_turn belongs to a footprint")
            o = traj_opts(inf["dim"], inf["step"], **opts)
            _check(self.L.gpis_traj_optimize(self.h, field.h, C.byref(o), C.c_void_p(stream)), "gpis_traj_optimize")
            return self
        o, wt = traj_body_opts(inf["dim"], inf["step"], max(footprint.info()["m"], 1), **opts)   # (an empty one: the call refuses it)
        wt = wt if w_turn is None else float(w_turn)
        _check(self.L.gpis_smooth_body_optimize(self.h, field.h, footprint.h, C.byref(o), C.c_float(wt), C.c_void_p(stream)),
               "gpis_smooth_body_optimize")
        return self

    def body_result(self):
        """The body result of the last optimize() with a footprint (gpis_smooth_body_get): what body_clearance(footprint, field,
        clearance) returns on the result, kept by the same launch.  dict(D_min [m] f64, waypoint, ball, collides [m] i32)."""
        m = self.info()["m"]
        r = dict(D_min=np.zeros(m, np.float64), waypoint=np.zeros(m, np.int32), ball=np.zeros(m, np.int32), collides=np.zeros(m, np.int32))
        _check(self.L.gpis_smooth_body_get(self.h, _p(r["D_min"], C.c_double), _p(r["waypoint"], C.c_int), _p(r["ball"], C.c_int),
                                         _p(r["collides"], C.c_int)), "gpis_smooth_body_get")
        return r

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_traj_info(self.h, _p(out, C.c_double), out.size), "gpis_traj_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """dict of host copies of the last result: x [m, N, dim] f32, status [m] u8 (0 stopped by tol, 1 iteration cap, 2 no
        input), iterations [m] i32, length, smooth, obstacle, min_dist [m] f32, nonfinite [m] i32, collides [m] u8."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("trajectories hold no result")
        m = i["m"]
        r = dict(x=np.zeros((m, i["N"], i["dim"]), np.float32), status=np.zeros(m, np.uint8), iterations=np.zeros(m, np.int32),
                 length=np.zeros(m, np.float32), smooth=np.zeros(m, np.float32), obstacle=np.zeros(m, np.float32),
                 min_dist=np.zeros(m, np.float32), nonfinite=np.zeros(m, np.int32), collides=np.zeros(m, np.uint8))
        _check(self.L.gpis_traj_get(self.h, _p(r["x"]), _p(r["status"], C.c_ubyte), _p(r["iterations"], C.c_int), _p(r["length"]),
                                    _p(r["smooth"]), _p(r["obstacle"]), _p(r["min_dist"]), _p(r["nonfinite"], C.c_int),
                                    _p(r["collides"], C.c_ubyte)), "gpis_traj_get")
        return r

    def device_ptrs(self):
        """(d_x, d_fres, d_ires) device addresses of the last result (0 where there is none)."""
        a, b, c = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_traj_device(self.h, C.byref(a), C.byref(b), C.byref(c)), "gpis_traj_device")
        return a.value or 0, b.value or 0, c.value or 0

    TIMING_INFO_KEYS = ("timed", "time_ms", "controls_ms")

    def time(self, df=None, stream=0, **opts):
        """Speeds and times on the last result under speed and acceleration limits (gpis_timing_time).  df: a DistanceField for
        the clearance slow-down, or None.  opts: gpis_traj_timing_opts fields.  Returns a dict of host copies: v, t [m, N] f32,
        limiter [m, N] u8 (0 v_max, 1 lateral acceleration, 2 yaw rate, 3 clearance, 4 the v_min floor, 5 an end speed, 6 an
        acceleration cone, 7 a braking cone), status [m] u8 (0 timed, 2 no input, 3 a non-finite time), duration, max_speed,
        max_curvature [m] f32, limiter_counts [m, 8] i32."""
        i = self.info()
        if not i["valid"]:
            raise GpisError("trajectories hold no result")
        o = timing_opts(i["dim"], df._step() if df is not None else 1.0, **opts)
        _check(self.L.gpis_timing_time(self.h, df.h if df is not None else None, C.byref(o), C.c_void_p(stream)), "gpis_timing_time")
        return self.timing()

    def timing_info(self):
        """dict(timed, time_ms, controls_ms): whether a timing is held, host wall times of the last time() and controls()."""
        out = np.zeros(len(self.TIMING_INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_timing_info(self.h, _p(out, C.c_double), out.size), "gpis_timing_info")
        d = dict(zip(self.TIMING_INFO_KEYS, out.tolist()))
        d["timed"] = int(d["timed"])
        return d

    def timing(self):
        """The dict time() returned, again (gpis_timing_get)."""
        i = self.info()
        if not self.timing_info()["timed"]:
            raise GpisError("trajectories hold no timing")
        m, N = i["m"], i["N"]
        r = dict(v=np.zeros((m, N), np.float32), t=np.zeros((m, N), np.float32), limiter=np.zeros((m, N), np.uint8),
                 status=np.zeros(m, np.uint8), duration=np.zeros(m, np.float32), max_speed=np.zeros(m, np.float32),
                 max_curvature=np.zeros(m, np.float32), limiter_counts=np.zeros((m, 8), np.int32))
        _check(self.L.gpis_timing_get(self.h, _p(r["v"]), _p(r["t"]), _p(r["limiter"], C.c_ubyte), _p(r["status"], C.c_ubyte),
                                      _p(r["duration"]), _p(r["max_speed"]), _p(r["max_curvature"]),
                                      _p(r["limiter_counts"], C.c_int)), "gpis_timing_get")
        return r

    def controls(self, dt, T, t0=0.0, w_limit=0.0, min_move=1e-9):
        """Control sequences of the controller's model along the timed trajectories (gpis_timing_controls): (U [m, T, 2 / 4] f64,
        heading0 [m, 2], p0 [m, dim], clamped [m] i32) for a robot that starts at p0 facing heading0."""
        i = self.info()
        if not self.timing_info()["timed"]:
            raise GpisError("trajectories hold no timing")
        m, T = i["m"], int(T)
        nu = 4 if i["dim"] == 3 else 2
        U = np.zeros((m, max(T, 0), nu), np.float64)
        h0, p0, cl = np.zeros((m, 2), np.float64), np.zeros((m, i["dim"]), np.float64), np.zeros(m, np.int32)
        _check(self.L.gpis_timing_controls(self.h, float(dt), T, float(t0), float(w_limit), float(min_move), _p(U, C.c_double),
                                           _p(h0, C.c_double), _p(p0, C.c_double), _p(cl, C.c_int)), "gpis_timing_controls")
        return U, h0, p0, cl


    def check(self, obstacles, dt, steps, t0=0.0, t_begin=0.0, clearance=None, footprint=None):
        """The timed trajectories against an Obstacles (gpis_obst_check_timing): sampled at t0 + k dt, k = 0 .. steps, trajectory
        time 0 at the absolute time t_begin; between samples both bodies move in straight lines and the closest approach is
        taken in continuous time.  clearance None: the set's own.  Returns dict(min_sep, min_time [m] f64, min_obstacle,
        first_hit, collides [m] i32).  footprint: a Footprint in the point's place (gpis_timed_body_check): the body at its timed
        pose -- the heading of the segment it is on -- and every pair of a body ball and a moving ball; the dict gains min_ball."""
        m = self.info()["m"]
        if clearance is None:
            clearance = obstacles.get()["opts"]["clearance"]
        r = dict(min_sep=np.zeros(m, np.float64), min_time=np.zeros(m, np.float64), min_obstacle=np.zeros(m, np.int32),
                 first_hit=np.zeros(m, np.int32), collides=np.zeros(m, np.int32))
        if footprint is not None:
            r["min_ball"] = np.zeros(m, np.int32)
            _check(self.L.gpis_timed_body_check(self.h, obstacles.h, footprint.h, float(dt), int(steps), float(t0), float(t_begin),
                                                 float(clearance), _p(r["min_sep"], C.c_double), _p(r["min_time"], C.c_double),
                                                 _p(r["min_obstacle"], C.c_int), _p(r["min_ball"], C.c_int), _p(r["first_hit"], C.c_int),
                                                 _p(r["collides"], C.c_int)), "gpis_timed_body_check")
            return r
        _check(self.L.gpis_obst_check_timing(self.h, obstacles.h, float(dt), int(steps), float(t0), float(t_begin), float(clearance),
                                             _p(r["min_sep"], C.c_double), _p(r["min_time"], C.c_double), _p(r["min_obstacle"], C.c_int),
                                             _p(r["first_hit"], C.c_int), _p(r["collides"], C.c_int)), "gpis_obst_check_timing")
        return r

    def timed_states(self, dt, steps, t0=0.0, retimed=False):
        """The timed poses (gpis_timed_body_states): [m, steps + 1, dim + 2] f64 states (p, c, s) as Footprint.clearance takes
        them, at t0 + k dt, or with retimed=True at the own slot of every real slot k of the last schedule (dt and t0 are not
        read).  The heading is the chord's of the segment the position lies on.  Rows without a timing or a schedule are NaN."""
        i = self.info()
        out = np.zeros((i["m"], max(int(steps), 0) + 1, i["dim"] + 2), np.float64)
        _check(self.L.gpis_timed_body_states(self.h, float(dt), int(steps), float(t0), 1 if retimed else 0, _p(out, C.c_double)),
               "gpis_timed_body_states")
        return out

    OWN_LEN = 1280                                       # real slots of the longest schedule (1024 own slots + 255 pauses + 1)

    def retime(self, obstacles, t_begin=0.0, stream=0, footprint=None, **opts):
        """Re-time the timed trajectories so that they wait for the balls of an Obstacles to pass (gpis_retime_solve): the
        geometry and the timing stay, a schedule says for every real slot of `slot` seconds, counted from the absolute time
        t_begin, which own slot of the timed trajectory is played; the schedule that arrives first within max_pause pause slots
        is kept.  opts: gpis_retime_opts fields (slot, max_pause, clearance, press_on); clearance defaults to the set's own.
        footprint: a Footprint in the point's place (gpis_timed_body_retime): a pause holds the pose of its own slot, a play step
        goes from the pose of one own slot to the next.  Returns retimed()."""
        i = self.info()
        if not self.timing_info()["timed"]:
            raise GpisError("trajectories hold no timing")
        if "clearance" not in opts:
            opts = dict(opts, clearance=obstacles.get()["opts"]["clearance"])
        o = retime_opts(i["dim"], 1.0, **opts)
        if footprint is not None:
            _check(self.L.gpis_timed_body_retime(self.h, obstacles.h, footprint.h, float(t_begin), C.byref(o), C.c_void_p(stream)),
                   "gpis_timed_body_retime")
            return self.retimed()
        _check(self.L.gpis_retime_solve(self.h, obstacles.h, float(t_begin), C.byref(o), C.c_void_p(stream)), "gpis_retime_solve")
        return self.retimed()

    def retimed_body_balls(self):
        """The number of body balls the last schedule was solved for (gpis_timed_body_info): 0 after a point solve."""
        out = np.zeros(1, np.float64)
        _check(self.L.gpis_timed_body_info(self.h, _p(out, C.c_double), 1), "gpis_timed_body_info")
        return int(out[0])

    def retimed(self):
        """The last schedule (gpis_retime_get): dict(status [m] i32 (0 clear as timed, 1 re-timed with pauses, 2 no timing, 3 no
        schedule within max_pause, 4 too long for this slot), arrive, pauses, own_slots, first_pause [m] i32, own [m, 1280] i32
        (the own slot of every real slot), slot, max_pause, clearance, press_on, t_begin, ms)."""
        m = self.info()["m"]
        r = {k: np.zeros(m, np.int32) for k in ("status", "arrive", "pauses", "own_slots", "first_pause")}
        r["own"] = np.zeros((m, self.OWN_LEN), np.int32)
        o = gpis_retime_opts()
        inf = np.zeros(2, np.float64)
        _check(self.L.gpis_retime_get(self.h, _p(r["status"], C.c_int), _p(r["arrive"], C.c_int), _p(r["pauses"], C.c_int),
                                      _p(r["own_slots"], C.c_int), _p(r["first_pause"], C.c_int), _p(r["own"], C.c_int), C.byref(o),
                                      _p(inf, C.c_double)), "gpis_retime_get")
        r.update(slot=o.slot, max_pause=o.max_pause, clearance=o.clearance, press_on=o.press_on, t_begin=float(inf[0]), ms=float(inf[1]))
        return r

    def retimed_controls(self, T, k0=0, w_limit=0.0, min_move=1e-9):
        """controls() along the last schedule from real slot k0 on, dt = the schedule's slot (gpis_retime_controls): a paused
        step has no displacement and keeps the heading of the latest moving step.  (U [m, T, 2 / 4] f64, heading0 [m, 2],
        p0 [m, dim], clamped [m] i32)."""
        i = self.info()
        m, T = i["m"], int(T)
        nu = 4 if i["dim"] == 3 else 2
        U = np.zeros((m, max(T, 0), nu), np.float64)
        h0, p0, cl = np.zeros((m, 2), np.float64), np.zeros((m, i["dim"]), np.float64), np.zeros(m, np.int32)
        _check(self.L.gpis_retime_controls(self.h, T, int(k0), float(w_limit), float(min_move), _p(U, C.c_double), _p(h0, C.c_double),
                                           _p(p0, C.c_double), _p(cl, C.c_int)), "gpis_retime_controls")
        return U, h0, p0, cl

    def retimed_check(self, obstacles, steps, clearance=None, footprint=None):
        """check() along the last schedule (gpis_retime_check): the robot at the schedule's position of every real slot
        k = 0 .. steps, the balls of `obstacles` (any set of this dim: a newer detection may be checked against an old schedule)
        at the real slots from the schedule's t_begin.  clearance None: the set's own.  Returns check()'s dict, min_time in real
        time from t_begin.  footprint: a Footprint in the point's place (gpis_timed_body_retime_check); the dict gains min_ball."""
        m = self.info()["m"]
        if clearance is None:
            clearance = obstacles.get()["opts"]["clearance"]
        r = dict(min_sep=np.zeros(m, np.float64), min_time=np.zeros(m, np.float64), min_obstacle=np.zeros(m, np.int32),
                 first_hit=np.zeros(m, np.int32), collides=np.zeros(m, np.int32))
        if footprint is not None:
            r["min_ball"] = np.zeros(m, np.int32)
            _check(self.L.gpis_timed_body_retime_check(self.h, obstacles.h, footprint.h, int(steps), float(clearance), _p(r["min_sep"], C.c_double),
                                                 _p(r["min_time"], C.c_double), _p(r["min_obstacle"], C.c_int), _p(r["min_ball"], C.c_int),
                                                 _p(r["first_hit"], C.c_int), _p(r["collides"], C.c_int)), "gpis_timed_body_retime_check")
            return r
        _check(self.L.gpis_retime_check(self.h, obstacles.h, int(steps), float(clearance), _p(r["min_sep"], C.c_double),
                                        _p(r["min_time"], C.c_double), _p(r["min_obstacle"], C.c_int), _p(r["first_hit"], C.c_int),
                                        _p(r["collides"], C.c_int)), "gpis_retime_check")
        return r

    def body_clearance(self, footprint, field, clearance=0.0):
        """A Footprint along the waypoints of the last result on a DistanceField (gpis_body_traj_clearance): the heading of a
        waypoint is its chord's.  Returns dict(D_min [m] f64, waypoint, ball, collides [m] i32)."""
        m = self.info()["m"]
        r = dict(D_min=np.zeros(m, np.float64), waypoint=np.zeros(m, np.int32), ball=np.zeros(m, np.int32), collides=np.zeros(m, np.int32))
        _check(self.L.gpis_body_traj_clearance(self.h, field.h, footprint.h, float(clearance), _p(r["D_min"], C.c_double),
                                               _p(r["waypoint"], C.c_int), _p(r["ball"], C.c_int), _p(r["collides"], C.c_int)),
               "gpis_body_traj_clearance")
        return r


def timing_opts(dim, step, **opts):
    """gpis_traj_timing_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_timing_default_opts)
    with the given fields replaced."""
    o = gpis_traj_timing_opts()
    _check(lib().gpis_timing_default_opts(int(dim), float(step), C.byref(o)), "gpis_timing_default_opts")
    names = {f[0] for f in gpis_traj_timing_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown timing option %r" % k)
        setattr(o, k, v)
    return o


def retime_opts(dim, step, **opts):
    """gpis_retime_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_retime_default_opts) with
    the given fields replaced."""
    o = gpis_retime_opts()
    _check(lib().gpis_retime_default_opts(int(dim), float(step), C.byref(o)), "gpis_retime_default_opts")
    names = {f[0] for f in gpis_retime_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown retime option %r" % k)
        setattr(o, k, v)
    return o


def render_field_opts(dim, step, **opts):
    """gpis_render_field_opts of the library's defaults for `dim` and a field of lattice step `step`
    (gpis_render_field_default_opts) with the given fields replaced."""
    o = gpis_render_field_opts()
    _check(lib().gpis_render_field_default_opts(int(dim), float(step), C.byref(o)), "gpis_render_field_default_opts")
    names = {f[0] for f in gpis_render_field_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown field render option %r" % k)
        setattr(o, k, v)
    return o


def render_opts(dim, **opts):
    """gpis_render_opts of the library's defaults for `dim` (gpis_render_default_opts) with the given fields replaced."""
    o = gpis_render_opts()
    _check(lib().gpis_render_default_opts(int(dim), C.byref(o)), "gpis_render_default_opts")
    names = {f[0] for f in gpis_render_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown render option %r" % k)
        setattr(o, k, v)
    return o


class Renderer:
    """Result holder of the renderer (gpis_render_*): device buffers reused across calls."""

    INFO_KEYS = ("rays", "dim", "passes", "march_passes", "samples", "evals", "k4_ms", "hits",
                 "box_lo_x", "box_lo_y", "box_lo_z", "box_hi_x", "box_hi_y", "box_hi_z", "valid", "mq_ms", "field", "max_samples")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_render_create())
        if not self.h:
            raise GpisError("gpis_render_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_render_destroy(self.h)
            self.h = None

    __del__ = close

    def set_chunk(self, rays):
        """Rays per test() call within a pass (0 = default 2^22; results do not depend on it)."""
        _check(self.L.gpis_render_set_chunk(self.h, int(rays)), "gpis_render_set_chunk")

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_render_info(self.h, _p(out, C.c_double), out.size), "gpis_render_info")
        return dict(zip(self.INFO_KEYS, out.tolist()))

    def box(self):
        """(lo [3], hi [3]) float32: the clip box of the last render (the cluster cells' box grown by the search half-width)."""
        i = self.info()
        return (np.array([i["box_lo_x"], i["box_lo_y"], i["box_lo_z"]], np.float32),
                np.array([i["box_hi_x"], i["box_hi_y"], i["box_hi_z"]], np.float32))

    def set_field_tiles(self, on):
        """Thread-to-pixel mapping of the 3-D field kernel: 8 x 8 pixel tiles per wavefront (default) or consecutive rays; the
        results do not depend on it."""
        _check(self.L.gpis_render_set_field_tiles(self.h, int(bool(on))), "gpis_render_set_field_tiles")

    def get(self):
        """(depth [n], rec [n, 2(1+dim)] after a map render / [n, 1+dim] after a field render, status [n] u8): host copies of
        the last result."""
        i = self.info()
        n, d = int(i["rays"]), int(i["dim"])
        depth = np.zeros(n, dtype=np.float32)
        rec = np.zeros((n, (1 + d) if i["field"] else 2 * (1 + d)), dtype=np.float32)
        status = np.zeros(n, dtype=np.uint8)
        _check(self.L.gpis_render_get(self.h, _p(depth), _p(rec), _p(status, C.c_ubyte)), "gpis_render_get")
        return depth, rec, status

    def device_ptrs(self):
        a, b, c = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_render_device(self.h, C.byref(a), C.byref(b), C.byref(c)), "gpis_render_device")
        return a.value or 0, b.value or 0, c.value or 0


def locate_opts(dim, **opts):
    """gpis_locate_opts of the library's defaults for `dim` (gpis_locate_default_opts) with the given fields replaced."""
    o = gpis_locate_opts()
    _check(lib().gpis_locate_default_opts(int(dim), C.byref(o)), "gpis_locate_default_opts")
    names = {f[0] for f in gpis_locate_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown locate option %r" % k)
        setattr(o, k, v)
    return o


class Locator:
    """Result holder of the pose scorer (gpis_locate_*): device buffers reused across calls."""

    INFO_KEYS = ("held", "dim", "poses", "points", "ranked", "pixels", "ms")
    INT_KEYS = ("held", "dim", "poses", "points", "ranked", "pixels")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_locate_create())
        if not self.h:
            raise GpisError("gpis_locate_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_locate_destroy(self.h)
            self.h = None

    __del__ = close

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_locate_info(self.h, _p(out, C.c_double), out.size), "gpis_locate_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """(cost [m] f64, inliers [m] i32, order [ranked] i32) of the last call."""
        i = self.info()
        if not i["held"]:
            raise GpisError("locator holds no result")
        cost = np.zeros(i["poses"], dtype=np.float64)
        inliers = np.zeros(i["poses"], dtype=np.int32)
        order = np.zeros(i["ranked"], dtype=np.int32)
        _check(self.L.gpis_locate_get(self.h, _p(cost, C.c_double), _p(inliers, C.c_int), _p(order, C.c_int)), "gpis_locate_get")
        return cost, inliers, order

    def device_ptrs(self):
        """(d_cost, d_inliers) device addresses of the last result (valid until the next call)."""
        a, b = C.c_void_p(0), C.c_void_p(0)
        _check(self.L.gpis_locate_device(self.h, C.byref(a), C.byref(b)), "gpis_locate_device")
        return a.value or 0, b.value or 0


def pf_opts(dim, **opts):
    """gpis_pf_opts of the library's defaults for `dim` (gpis_pf_default_opts) with the given fields replaced; sigma_t takes a
    scalar or a sequence of `dim` values."""
    o = gpis_pf_opts()
    _check(lib().gpis_pf_default_opts(int(dim), C.byref(o)), "gpis_pf_default_opts")
    names = {f[0] for f in gpis_pf_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown particle-filter option %r" % k)
        if k == "sigma_t":
            v = np.broadcast_to(np.asarray(v, np.float64).ravel(), (int(dim),)) if np.ndim(v) == 0 else np.asarray(v, np.float64).ravel()
            if v.size not in (int(dim), 3):
                raise GpisError("sigma_t must have %d values" % int(dim))
            for a in range(3):
                o.sigma_t[a] = float(v[a]) if a < v.size else 0.0
        else:
            setattr(o, k, v)
    return o


class ParticleFilter:
    """Monte-Carlo localisation against a DistanceField, resident on the device (gpis_pf_*): init from float32 poses, then
    predict / update_scan or update_depth per frame; an update returns the estimate, and only that leaves the device."""

    INFO_KEYS = ("inited", "dim", "particles", "tick", "points", "pixels", "updates", "resamplings", "resampled", "neff", "ms")
    INT_KEYS = INFO_KEYS[:9]
    PTR_KEYS = ("state", "poses", "L", "q", "cost", "inliers", "ancestors")

    def __init__(self, **opts):
        """opts: gpis_pf_opts fields that replace the defaults in every call of this filter."""
        self.L = lib()
        if not hasattr(self.L, "gpis_pf_create"):
            raise GpisError("the native library has no particle filter (gpis_pf_create)")
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_pf_create())
        if not self.h:
            raise GpisError("gpis_pf_create failed")
        self.opts = dict(opts)
        self.dim = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_pf_destroy(self.h)
            self.h = None

    __del__ = close

    def _opts(self, opts):
        d = dict(self.opts)
        d.update(opts)
        return pf_opts(self.dim, **d)

    def init(self, poses, seed=0):
        """The particle set from float32 poses [m, 6] (2-D) / [m, 12] (3-D); L = 0, tick = 0."""
        poses = np.ascontiguousarray(poses, dtype=np.float32)
        if poses.ndim != 2 or poses.shape[1] not in (6, 12) or poses.shape[0] < 1:
            raise GpisError("poses must be [m, 6] or [m, 12] with m >= 1")
        dim = 3 if poses.shape[1] == 12 else 2
        _check(self.L.gpis_pf_init(self.h, dim, _p(poses), poses.shape[0], C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF)), "gpis_pf_init")
        self.dim = dim
        return self

    def motion(self, motion):
        """The relative pose [t, R] (float64 [6] / [12]) of `motion`: that layout itself, (dx, dy, dtheta) in 2-D, or
        (d [3], rotvec [3]) in 3-D."""
        if self.dim == 3 and len(motion) == 2:
            d, w = (np.asarray(v, np.float64).ravel() for v in motion)
            if d.size != 3 or w.size != 3:
                raise GpisError("a 3-D motion is (d [3], rotvec [3]) or a pose [12]")
            return np.concatenate([d, _exp_so3(w).T.ravel()])
        mo = np.asarray(motion, np.float64).ravel()
        if self.dim == 2 and mo.size == 3:
            c, s = math.cos(float(mo[2])), math.sin(float(mo[2]))
            return np.array([mo[0], mo[1], c, s, -s, c], np.float64)
        if mo.size != (12 if self.dim == 3 else 6):
            raise GpisError("bad motion for a %d-D filter" % self.dim)
        return np.ascontiguousarray(mo)

    def predict(self, motion, stream=None, **opts):
        """Move every particle by `motion` (see motion()) in its own frame plus noise (sigma_t, sigma_r)."""
        if not self.dim:
            raise GpisError("predict before init")
        mo = self.motion(motion)
        o = self._opts(opts)
        _check(self.L.gpis_pf_predict(self.h, _p(mo, C.c_double), C.byref(o), stream), "gpis_pf_predict")

    def update_scan(self, field, thetas, ranges, off2, stream=None, **opts):
        """Weigh the set against a laser scan in `field` (gpis2_pf_update_scan), estimate, resample if N_eff asks for it.
        Returns estimate()."""
        return self._update_scan(None, field, thetas, ranges, off2, stream, opts)

    def update_depth(self, field, depth, cam6, stream=None, **opts):
        """update_scan for a depth image (gpis3_pf_update_depth)."""
        return self._update_depth(None, None, field, depth, cam6, stream, opts)

    def _update_scan(self, map_h, field, thetas, ranges, off2, stream, opts):
        thetas, ranges, off = _scan_frame("update_scan", thetas, ranges, off2, map_h)
        o = self._opts(opts)
        _check(self.L.gpis2_pf_update_scan(map_h, field.h, self.h, _p(thetas), _p(ranges), thetas.size, off, C.byref(o), stream),
               "gpis2_pf_update_scan")
        return self.estimate()

    def _update_depth(self, map_h, map_wh, field, depth, cam6, stream, opts):
        depth, cam = _depth_frame("update_depth", depth, cam6, map_h, map_wh)
        o = self._opts(opts)
        _check(self.L.gpis3_pf_update_depth(map_h, field.h, self.h, cam, _p(depth), C.byref(o), stream), "gpis3_pf_update_depth")
        return self.estimate()

    def resample(self, stream=None):
        """Systematic resampling from the last update's weights (uniform after init), whatever N_eff says."""
        _check(self.L.gpis_pf_resample(self.h, stream), "gpis_pf_resample")

    def estimate(self):
        """dict of the last update: pose (float64 [6] / [12] = [t, R]), neff, T, Th, S2 (Python ints), resampled."""
        pose = np.zeros(12 if self.dim == 3 else 6, dtype=np.float64)
        neff, tot, rs = C.c_double(0.0), (C.c_ulonglong * 3)(), C.c_int(0)
        _check(self.L.gpis_pf_estimate(self.h, _p(pose, C.c_double), C.byref(neff), tot, C.byref(rs)), "gpis_pf_estimate")
        return dict(pose=pose, neff=neff.value, T=int(tot[0]), Th=int(tot[1]), S2=int(tot[2]), resampled=bool(rs.value))

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_pf_info(self.h, _p(out, C.c_double), out.size), "gpis_pf_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """dict of host copies: state [m, 4 / 7] f64, L [m] f64, q [m] u64, cost [m] f64, inliers [m] i32, ancestors [m] i32,
        poses [m, 6 / 12] f32."""
        i = self.info()
        if not i["inited"]:
            raise GpisError("the particle filter holds no set")
        m, d3 = i["particles"], i["dim"] == 3
        out = dict(state=np.zeros((m, 7 if d3 else 4), np.float64), L=np.zeros(m, np.float64), q=np.zeros(m, np.uint64),
                   cost=np.zeros(m, np.float64), inliers=np.zeros(m, np.int32), ancestors=np.zeros(m, np.int32),
                   poses=np.zeros((m, 12 if d3 else 6), np.float32))
        _check(self.L.gpis_pf_get(self.h, _p(out["state"], C.c_double), _p(out["L"], C.c_double), _p(out["q"], C.c_ulonglong),
                                  _p(out["cost"], C.c_double), _p(out["inliers"], C.c_int), _p(out["ancestors"], C.c_int),
                                  _p(out["poses"])), "gpis_pf_get")
        return out

    def poses(self):
        """The float32 poses [m, 6 / 12] the scorer reads."""
        i = self.info()
        if not i["inited"]:
            raise GpisError("the particle filter holds no set")
        out = np.zeros((i["particles"], 12 if i["dim"] == 3 else 6), np.float32)
        _check(self.L.gpis_pf_get(self.h, None, None, None, None, None, None, _p(out)), "gpis_pf_get")
        return out

    def device_ptrs(self):
        """dict of device addresses (state, poses, L, q, cost, inliers, ancestors), valid until the next init or resampling."""
        a = (C.c_void_p * 7)()
        _check(self.L.gpis_pf_device(self.h, a, 7), "gpis_pf_device")
        return dict(zip(self.PTR_KEYS, [v or 0 for v in a]))


def mppi_opts(dim, step=1.0, **opts):
    """gpis_mppi_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_mppi_default_opts) with the
    given fields replaced; `lam` stands for lambda; sigma, umin and umax take a sequence of 2 (dim 2) or 4 values."""
    o = gpis_mppi_opts()
    _check(lib().gpis_mppi_default_opts(int(dim), float(step), C.byref(o)), "gpis_mppi_default_opts")
    names = {f[0] for f in gpis_mppi_opts._fields_}
    nu = 4 if int(dim) == 3 else 2
    for k, v in opts.items():
        k = "lambda" if k == "lam" else k
        if k not in names:
            raise GpisError("unknown controller option %r" % k)
        if k in ("sigma", "umin", "umax"):
            v = np.asarray(v, np.float64).ravel()
            if v.size not in (nu, 4):
                raise GpisError("%s must have %d values" % (k, nu))
            a = getattr(o, k)
            for u in range(4):
                a[u] = float(v[u]) if u < v.size else 0.0
        else:
            setattr(o, k, float(v))
    return o


def obst_opts(dim, step, **opts):
    """gpis_obst_opts of the library's defaults for `dim` and a field of lattice step `step` (gpis_obst_default_opts) with the
    given fields replaced."""
    o = gpis_obst_opts()
    _check(lib().gpis_obst_default_opts(int(dim), float(step), C.byref(o)), "gpis_obst_default_opts")
    names = {f[0] for f in gpis_obst_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown obstacle option %r" % k)
        setattr(o, k, float(v))
    return o


class Obstacles:
    """A set of at most 256 moving balls (gpis_obst_*): centres, constant velocities and radii in double with one epoch, and the
    cost options of their term in a Controller's rollouts.  The set may be changed or closed between any two calls that take it."""

    MAX = 256
    INFO_KEYS = ("inited", "dim", "n", "epoch", "device")

    def __init__(self, dim, step, **opts):
        """dim and the lattice step of the field give the default options (obst_opts); opts replace them."""
        self.L = lib()
        if not hasattr(self.L, "gpis_obst_create"):
            raise GpisError("the native library has no moving obstacles (gpis_obst_create)")
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_obst_create())
        if not self.h:
            raise GpisError("gpis_obst_create failed")
        self.dim, self.step = int(dim), float(step)
        self.set_opts(**opts)

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_obst_destroy(self.h)
            self.h = None

    __del__ = close

    def set_opts(self, **opts):
        """Replace the options by the defaults with `opts` over them."""
        o = obst_opts(self.dim, self.step, **opts)
        _check(self.L.gpis_obst_set_opts(self.h, C.byref(o)), "gpis_obst_set_opts")
        return self

    def set(self, centre, velocity, radius, epoch=0.0):
        """centre, velocity [n, dim], radius [n] (n = 0 empties the set); epoch: the absolute time at which the centres hold."""
        c = np.ascontiguousarray(centre, dtype=np.float64).reshape(-1, self.dim)
        v = np.ascontiguousarray(velocity, dtype=np.float64).reshape(-1, self.dim)
        r = np.ascontiguousarray(radius, dtype=np.float64).ravel()
        if not (c.shape[0] == v.shape[0] == r.size):
            raise GpisError("centre, velocity and radius must have one row per ball")
        _check(self.L.gpis_obst_set(self.h, self.dim, r.size, _p(c, C.c_double), _p(v, C.c_double), _p(r, C.c_double), float(epoch)),
               "gpis_obst_set")
        return self

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_obst_info(self.h, _p(out, C.c_double), out.size), "gpis_obst_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in ("inited", "dim", "n", "device"):
            d[k] = int(d[k])
        return d

    def get(self):
        """dict(centre [n, dim], velocity [n, dim], radius [n], epoch, opts: dict of the four options)."""
        i = self.info()
        n, dim = i["n"], i["dim"] or self.dim
        c, v, r, o = np.zeros((n, dim), np.float64), np.zeros((n, dim), np.float64), np.zeros(n, np.float64), gpis_obst_opts()
        _check(self.L.gpis_obst_get(self.h, _p(c, C.c_double), _p(v, C.c_double), _p(r, C.c_double), C.byref(o)), "gpis_obst_get")
        return dict(centre=c, velocity=v, radius=r, epoch=i["epoch"], opts={f[0]: getattr(o, f[0]) for f in gpis_obst_opts._fields_})

    def at(self, t):
        """The centres [n, dim] at absolute time t (gpis_obst_at; computed on the host)."""
        i = self.info()
        out = np.zeros((i["n"], i["dim"] or self.dim), np.float64)
        _check(self.L.gpis_obst_at(self.h, float(t), _p(out, C.c_double)), "gpis_obst_at")
        return out


def states_from_poses(poses, dim=None):
    """States [n, dim + 2] = (p, c, s) of poses [t, R] of 6 (2-D) or 12 (3-D) values each: (c, s) = (R[0], R[1]) divided by its
    norm, as gpis_mppi_step takes its start."""
    P = np.asarray(poses, dtype=np.float64)
    if dim is None:
        dim = 3 if P.shape[-1] == 12 else 2
    P = P.reshape(-1, 12 if dim == 3 else 6)
    out = np.zeros((P.shape[0], dim + 2), np.float64)
    for i, p in enumerate(P):
        r0, r1 = float(p[dim]), float(p[dim + 1])
        n = math.sqrt(r0 * r0 + r1 * r1)
        out[i, :dim] = p[:dim]
        out[i, dim], out[i, dim + 1] = r0 / n, r1 / n
    return out


class Footprint:
    """The robot's footprint (gpis_body_*): at most 16 balls fixed to the robot, offsets in the body frame (x forward, y left, z
    up) and radii in double.  It may be changed or closed between any two calls that take it."""

    MAX = 16
    INFO_KEYS = ("inited", "dim", "m", "device")

    def __init__(self, dim):
        self.L = lib()
        if not hasattr(self.L, "gpis_body_create"):
            raise GpisError("the native library has no footprints (gpis_body_create)")
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_body_create())
        if not self.h:
            raise GpisError("gpis_body_create failed")
        self.dim = int(dim)

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_body_destroy(self.h)
            self.h = None

    __del__ = close

    @staticmethod
    def box_table(length, width, n):
        """(offset [n, 2], radius [n]) of n equal discs along the x axis whose union covers a length x width rectangle centred on
        the reference point: centres at -length / 2 + (j + 1 / 2) length / n, radius hypot(width / 2, length / (2 n)).  Host numpy."""
        n = int(n)
        if n < 1 or not (length > 0 and width > 0):
            raise GpisError("box needs n >= 1 and positive sides")
        off = np.zeros((n, 2), np.float64)
        off[:, 0] = -0.5 * float(length) + (np.arange(n, dtype=np.float64) + 0.5) * (float(length) / n)
        return off, np.full(n, math.hypot(0.5 * float(width), float(length) / (2.0 * n)), np.float64)

    @classmethod
    def box(cls, length, width, n):
        """A 2-D Footprint holding box_table(length, width, n)."""
        off, rad = cls.box_table(length, width, n)
        return cls(2).set(off, rad)

    def set(self, offset, radius):
        """offset [m, dim], radius [m] (m = 0 empties the footprint)."""
        o = np.ascontiguousarray(offset, dtype=np.float64).reshape(-1, self.dim)
        r = np.ascontiguousarray(radius, dtype=np.float64).ravel()
        if o.shape[0] != r.size:
            raise GpisError("offset and radius must have one row per ball")
        _check(self.L.gpis_body_set(self.h, self.dim, r.size, _p(o, C.c_double), _p(r, C.c_double)), "gpis_body_set")
        return self

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_body_info(self.h, _p(out, C.c_double), out.size), "gpis_body_info")
        return {k: int(v) for k, v in zip(self.INFO_KEYS, out.tolist())}

    def get(self):
        """dict(offset [m, dim], radius [m])."""
        i = self.info()
        m, dim = i["m"], i["dim"] or self.dim
        o, r = np.zeros((m, dim), np.float64), np.zeros(m, np.float64)
        _check(self.L.gpis_body_get(self.h, _p(o, C.c_double), _p(r, C.c_double)), "gpis_body_get")
        return dict(offset=o, radius=r)

    def clearance(self, field, states, clearance=0.0, stream=None):
        """The body rule at states [n, dim + 2] = (p, c, s) with unit headings, on a DistanceField (gpis_body_clearance).  Returns
        dict(D [n] f64: the least of the balls' sampled distances less their radii, NaN off the lattice; ball [n] i32: which
        ball; below: states with D < clearance; off: states off the lattice; least: the index of the least D, -1 if none)."""
        S = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, self.dim + 2)
        n = S.shape[0]
        D, b, cnt = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(3, np.int32)
        _check(self.L.gpis_body_clearance(field.h, self.h, _p(S, C.c_double), n, float(clearance), _p(D, C.c_double), _p(b, C.c_int),
                                          _p(cnt, C.c_int), stream), "gpis_body_clearance")
        return dict(D=D, ball=b, below=int(cnt[0]), off=int(cnt[1]), least=int(cnt[2]))


class Controller:
    """Sampled model-predictive control (MPPI) against a DistanceField, resident on the device (gpis_mppi_*): init, then per
    control period step (or DistanceField.control) and shift; a step returns the next command, and only a small block leaves
    the device."""

    INFO_KEYS = ("inited", "dim", "rollouts", "horizon", "tick", "steps", "have_step", "ms")
    INT_KEYS = INFO_KEYS[:7]
    PTR_KEYS = ("U", "J", "q", "hits", "nominal_states")
    STAT_KEYS = ("Jmin", "best", "neff", "T", "Th", "S2", "hits", "nominal_cost", "nominal_hits", "have_step")

    def __init__(self, **opts):
        """opts: gpis_mppi_opts fields that replace the defaults in every step of this controller."""
        self.L = lib()
        if not hasattr(self.L, "gpis_mppi_create"):
            raise GpisError("the native library has no sampling controller (gpis_mppi_create)")
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_mppi_create())
        if not self.h:
            raise GpisError("gpis_mppi_create failed")
        self.opts = dict(opts)
        self.dim = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_mppi_destroy(self.h)
            self.h = None

    __del__ = close

    def init(self, dim, K, T, seed=0):
        """K rollouts of T steps for a field of `dim`; the nominal sequence zero, tick = 0."""
        _check(self.L.gpis_mppi_init(self.h, int(dim), int(K), int(T), C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF)), "gpis_mppi_init")
        self.dim = int(dim)
        return self

    def set_nominal(self, U):
        """Replace the nominal sequence by U [T, 2 / 4]."""
        i = self.info()
        if not i["inited"]:
            raise GpisError("set_nominal before init")
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.size != i["horizon"] * (4 if i["dim"] == 3 else 2):
            raise GpisError("U must be [T, %d]" % (4 if i["dim"] == 3 else 2))
        _check(self.L.gpis_mppi_set_nominal(self.h, _p(U, C.c_double)), "gpis_mppi_set_nominal")

    def follow(self, traj, index, dt=None, t0=0.0, w_limit=0.0, min_move=1e-9, retimed=False, k0=0):
        """Replace the nominal sequence by the control sequence of trajectory `index` of a timed Trajectories from time t0 on, in
        steps of dt (gpis_timing_follow); the sequence is computed on the device and stays there.  retimed=True: along the
        trajectory's last schedule from real slot k0 on, in steps of the schedule's slot (gpis_retime_follow; dt and t0 are not
        given: the controller is meant to run at dt = slot).  Returns (p0 [dim], heading0 [2]): where the sequence starts and
        which way it faces."""
        if not self.dim:
            raise GpisError("follow before init")
        p0, h0 = np.zeros(self.dim, np.float64), np.zeros(2, np.float64)
        if retimed:
            if dt is not None or t0 != 0.0:
                raise GpisError("a schedule runs in its own slots from k0 on: dt and t0 are not given")
            _check(self.L.gpis_retime_follow(self.h, traj.h, int(index), int(k0), float(w_limit), float(min_move),
                                             _p(h0, C.c_double), _p(p0, C.c_double)), "gpis_retime_follow")
            return p0, h0
        if dt is None or k0 != 0:
            raise GpisError("follow needs dt; k0 belongs to a schedule")
        _check(self.L.gpis_timing_follow(self.h, traj.h, int(index), float(dt), float(t0), float(w_limit), float(min_move),
                                         _p(h0, C.c_double), _p(p0, C.c_double)), "gpis_timing_follow")
        return p0, h0

    def step(self, field, pose, goal=None, planner=None, stream=None, obstacles=None, t=0.0, footprint=None, **opts):
        """gpis_mppi_step, or with `obstacles` (an Obstacles) gpis_obst_mppi_step at absolute time t, or with `footprint` (a
        Footprint) gpis_body_mppi_step: see DistanceField.control."""
        if not self.dim:
            raise GpisError("step before init")
        if (goal is None) == (planner is None):
            raise GpisError("exactly one of goal and planner gives the terminal cost")
        pose = np.ascontiguousarray(pose, dtype=np.float64).ravel()
        if pose.size != (12 if self.dim == 3 else 6):
            raise GpisError("pose must have %d elements" % (12 if self.dim == 3 else 6))
        g = None
        if goal is not None:
            g = np.ascontiguousarray(goal, dtype=np.float64).ravel()
            if g.size != self.dim:
                raise GpisError("goal must have %d elements" % self.dim)
        d = dict(self.opts)
        d.update(opts)
        o = mppi_opts(self.dim, field._step(), **d)
        u0 = np.zeros(4 if self.dim == 3 else 2, dtype=np.float64)
        if footprint is not None:
            _check(self.L.gpis_body_mppi_step(self.h, field.h, planner.h if planner is not None else None, footprint.h,
                                              obstacles.h if obstacles is not None else None, float(t), _p(pose, C.c_double),
                                              _p(g, C.c_double) if g is not None else None, C.byref(o), _p(u0, C.c_double), stream),
                   "gpis_body_mppi_step")
            return u0, self.stats()
        if obstacles is not None:
            _check(self.L.gpis_obst_mppi_step(self.h, field.h, planner.h if planner is not None else None, obstacles.h, float(t),
                                              _p(pose, C.c_double), _p(g, C.c_double) if g is not None else None, C.byref(o),
                                              _p(u0, C.c_double), stream), "gpis_obst_mppi_step")
            return u0, self.stats()
        _check(self.L.gpis_mppi_step(self.h, field.h, planner.h if planner is not None else None, _p(pose, C.c_double),
                                     _p(g, C.c_double) if g is not None else None, C.byref(o), _p(u0, C.c_double), stream),
               "gpis_mppi_step")
        return u0, self.stats()

    def obstacle_stats(self):
        """dict of the last step's view of the moving balls (gpis_obst_mppi_get): dyn_hit_rollouts, nominal_dyn_hits,
        nominal_min_sep, n.  After a step without balls: 0, 0, inf, 0."""
        out = np.zeros(4, dtype=np.float64)
        _check(self.L.gpis_obst_mppi_get(self.h, None, None, _p(out, C.c_double)), "gpis_obst_mppi_get")
        return dict(dyn_hit_rollouts=int(out[0]), nominal_dyn_hits=int(out[1]), nominal_min_sep=float(out[2]), n=int(out[3]))

    def get_obstacle(self):
        """dict(dyn_hits [K] i32: each rollout's steps nearer a ball than the set's clearance; min_sep [K] f64: its least
        separation) of the last step."""
        i = self.info()
        if not i["inited"]:
            raise GpisError("the controller is not initialised")
        out = dict(dyn_hits=np.zeros(i["rollouts"], np.int32), min_sep=np.zeros(i["rollouts"], np.float64))
        _check(self.L.gpis_obst_mppi_get(self.h, _p(out["dyn_hits"], C.c_int), _p(out["min_sep"], C.c_double), None), "gpis_obst_mppi_get")
        return out

    def shift(self):
        """Drop the first row of the nominal sequence (the command that has been applied); the last row stays."""
        _check(self.L.gpis_mppi_shift(self.h), "gpis_mppi_shift")

    def stats(self):
        """dict of the last step: Jmin, best, neff, T, Th, S2 (Python ints), hits (rollouts that touched an obstacle),
        nominal_cost, nominal_hits."""
        out = np.zeros(10, dtype=np.float64)
        _check(self.L.gpis_mppi_get(self.h, None, None, None, None, None, _p(out, C.c_double)), "gpis_mppi_get")
        d = dict(zip(self.STAT_KEYS, out.tolist()))
        for k in ("best", "T", "Th", "S2", "hits", "nominal_hits", "have_step"):
            d[k] = int(d[k])
        return d

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_mppi_info(self.h, _p(out, C.c_double), out.size), "gpis_mppi_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """dict of host copies: U [T, 2 / 4] f64 (the nominal sequence), and of the last step J [K] f64, q [K] u64, hits [K]
        i32, nominal_states [T + 1, dim + 2] f64, stats (see stats())."""
        i = self.info()
        if not i["inited"]:
            raise GpisError("the controller is not initialised")
        K, T, nu, ns = i["rollouts"], i["horizon"], 4 if i["dim"] == 3 else 2, i["dim"] + 2
        out = dict(U=np.zeros((T, nu), np.float64), J=np.zeros(K, np.float64), q=np.zeros(K, np.uint64), hits=np.zeros(K, np.int32),
                   nominal_states=np.zeros((T + 1, ns), np.float64))
        st = np.zeros(10, dtype=np.float64)
        _check(self.L.gpis_mppi_get(self.h, _p(out["U"], C.c_double), _p(out["J"], C.c_double), _p(out["q"], C.c_ulonglong),
                                    _p(out["hits"], C.c_int), _p(out["nominal_states"], C.c_double), _p(st, C.c_double)), "gpis_mppi_get")
        d = dict(zip(self.STAT_KEYS, st.tolist()))
        for k in ("best", "T", "Th", "S2", "hits", "nominal_hits", "have_step"):
            d[k] = int(d[k])
        out["stats"] = d
        return out

    def device_ptrs(self):
        """dict of device addresses (U, J, q, hits, nominal_states); U changes halves with every step and shift."""
        a = (C.c_void_p * 5)()
        _check(self.L.gpis_mppi_device(self.h, a, 5), "gpis_mppi_device")
        return dict(zip(self.PTR_KEYS, [v or 0 for v in a]))


def pose_grid2(xs, ys, thetas):
    """[m, 6] float32 poses [t(2), R(4)] of every (x, y, angle): the angle is the slowest axis, then y, then x; cos and sin in
    float64, cast."""
    xs, ys, th = (np.asarray(v, np.float64).ravel() for v in (xs, ys, thetas))
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    c, s = np.cos(T), np.sin(T)
    return np.stack([X, Y, c, s, -s, c], axis=-1).reshape(-1, 6).astype(np.float32)


def _exp_so3(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def pose_grid3(pose12, offsets, rotvecs):
    """[a b, 12] float32 poses [t(3), R(9)] around pose12: Exp(rotvec) R and t + offset for every offset [a, 3] and rotation
    vector [b, 3], in float64, cast; the rotation vector is the slowest axis."""
    P = np.asarray(pose12, np.float64).ravel()
    t, R = P[:3], P[3:].reshape(3, 3).T
    off = np.asarray(offsets, np.float64).reshape(-1, 3)
    out = []
    for w in np.asarray(rotvecs, np.float64).reshape(-1, 3):
        Rw = _exp_so3(w) @ R
        out.append(np.concatenate([t[None, :] + off, np.tile(Rw.T.ravel(), (off.shape[0], 1))], axis=1))
    return np.concatenate(out, axis=0).astype(np.float32)


def track_opts(dim, **opts):
    """gpis_track_opts of the library's defaults for `dim` (gpis_track_default_opts) with the given fields replaced."""
    o = gpis_track_opts()
    _check(lib().gpis_track_default_opts(int(dim), C.byref(o)), "gpis_track_default_opts")
    names = {f[0] for f in gpis_track_opts._fields_}
    for k, v in opts.items():
        if k not in names:
            raise GpisError("unknown track option %r" % k)
        setattr(o, k, v)
    return o


class Tracker:
    """Result holder of the tracker (gpis_track_*): device buffers reused across calls."""

    INFO_KEYS = ("status", "iterations", "passes", "points", "inliers", "cost0", "cost", "pass_ms", "k4_ms", "valid", "dim",
                 "pixels", "evals")
    INT_KEYS = ("status", "iterations", "passes", "points", "inliers", "valid", "dim", "pixels", "evals")

    def __init__(self):
        self.L = lib()
        if self.L.gpis_device_count() < 1:
            raise GpisError("no HIP device: gpismap_amd has no CPU fallback")
        self.h = C.c_void_p(self.L.gpis_track_create())
        if not self.h:
            raise GpisError("gpis_track_create failed")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_track_destroy(self.h)
            self.h = None

    __del__ = close

    def set_chunk(self, points):
        """Points per test() call within a pass (0 = default 2^22; results do not depend on it)."""
        _check(self.L.gpis_track_set_chunk(self.h, int(points)), "gpis_track_set_chunk")

    def info(self):
        out = np.zeros(len(self.INFO_KEYS), dtype=np.float64)
        _check(self.L.gpis_track_info(self.h, _p(out, C.c_double), out.size), "gpis_track_info")
        d = dict(zip(self.INFO_KEYS, out.tolist()))
        for k in self.INT_KEYS:
            d[k] = int(d[k])
        return d

    def get(self):
        """(H [n, n] f64, b [n] f64, resid [pixels] f32) of the last call (n = 6 / 3)."""
        i = self.info()
        n = 6 if i["dim"] == 3 else 3
        H = np.zeros((n, n), dtype=np.float64)
        b = np.zeros(n, dtype=np.float64)
        resid = np.zeros(i["pixels"], dtype=np.float32)
        _check(self.L.gpis_track_get(self.h, _p(H, C.c_double), _p(b, C.c_double), _p(resid)), "gpis_track_get")
        return H, b, resid

    def result(self):
        """info() with "H", "b" and "resid" of the last call."""
        d = self.info()
        d["H"], d["b"], d["resid"] = self.get()
        return d


class ObsGP:
    """Kernel-level K1/K2: device-resident observation GP."""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p(self.L.gpis_obsgp_create())
        if not self.h:
            raise GpisError("gpis_obsgp_create failed (no HIP device?)")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_obsgp_destroy(self.h)
            self.h = None

    __del__ = close

    def train2d(self, vu, f, ni, nj):
        vu = np.ascontiguousarray(vu, dtype=np.float32)
        f = np.ascontiguousarray(f, dtype=np.float32)
        _check(self.L.gpis_obsgp_train2d(self.h, _p(vu), _p(f), ni, nj), "gpis_obsgp_train2d")

    def train1d(self, theta, f):
        theta = np.ascontiguousarray(theta, dtype=np.float32)
        f = np.ascontiguousarray(f, dtype=np.float32)
        _check(self.L.gpis_obsgp_train1d(self.h, _p(theta), _p(f), theta.size), "gpis_obsgp_train1d")

    def query(self, q, val0=0.0):
        q = np.ascontiguousarray(q, dtype=np.float32)
        n = q.shape[0]
        val = np.full(n, val0, dtype=np.float32)
        var = np.zeros(n, dtype=np.float32)
        _check(self.L.gpis_obsgp_query(self.h, _p(q), n, _p(val), _p(var)), "gpis_obsgp_query")
        return val, var

    def query_route(self, route, q, val0=0.0):
        """The batch through route 0 (query), 1 (stage_q + query_staged) or 2 (stage_qb + query_staged_b_async + wait_b);
        routes 1 and 2 start from val = 0 whatever val0 says."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        n = q.shape[0]
        val = np.full(n, val0, dtype=np.float32)
        var = np.zeros(n, dtype=np.float32)
        _check(self.L.gpis_obsgp_query_route(self.h, route, _p(q), n, _p(val), _p(var)), "gpis_obsgp_query_route")
        return val, var

    def query_begin_b(self, q):
        """First half of route 2: the batch is left pending on the second staging set (collect with query_end_b)."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        _check(self.L.gpis_obsgp_query_route(self.h, 3, _p(q), q.shape[0], None, None), "gpis_obsgp_query_route")
        return q.shape[0]

    def query_end_b(self, n):
        val = np.zeros(n, dtype=np.float32)
        var = np.zeros(n, dtype=np.float32)
        _check(self.L.gpis_obsgp_query_route(self.h, 4, None, n, _p(val), _p(var)), "gpis_obsgp_query_route")
        return val, var

    def pending(self):
        """True while a batch of the second staging set is issued and not yet waited for."""
        return self.L.gpis_obsgp_pending(self.h) == 1

    def num_groups(self):
        return self.L.gpis_obsgp_num_groups(self.h)

    def group(self, g):
        n = C.c_int(0)
        x = np.zeros((64, 2), dtype=np.float32)
        alpha = np.zeros(64, dtype=np.float32)
        L = np.zeros((64, 64), dtype=np.float32)  # column-major on the device: L[c, r]
        _check(self.L.gpis_obsgp_get_group(self.h, g, C.byref(n), _p(x), _p(alpha), _p(L)), "gpis_obsgp_get_group")
        return n.value, x, alpha, L.T.copy()


class OnGPIS:
    """Kernel-level K6/K3/K4: batched cluster training and prediction."""

    def __init__(self, dim, scale, keep_factor=False, fused=True):
        """keep_factor: models of at most 256 rows (trained on chip) also keep L / alpha / gidx for model();
        fused=False: every cluster takes the separate training kernels."""
        self.L = lib()
        self.dim = dim
        self.h = C.c_void_p(self.L.gpis_ongpis_create(dim, float(scale)))
        if not self.h:
            raise GpisError("gpis_ongpis_create failed (no HIP device?)")
        _check(self.L.gpis_ongpis_set_keep_factor(self.h, 1 if keep_factor else 0), "gpis_ongpis_set_keep_factor")
        _check(self.L.gpis_ongpis_set_fused(self.h, 1 if fused else 0), "gpis_ongpis_set_fused")

    def close(self):
        if getattr(self, "h", None):
            self.L.gpis_ongpis_destroy(self.h)
            self.h = None

    __del__ = close

    def train(self, points9, off, ids):
        """points9: [9, npts] SoA; off: [ncl+1]; ids: concatenated point ids.  Returns model slots."""
        points9 = np.ascontiguousarray(points9, dtype=np.float32)
        off = np.ascontiguousarray(off, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        ncl = off.size - 1
        models = np.zeros(ncl, dtype=np.int32)
        _check(self.L.gpis_ongpis_train(self.h, _p(points9), points9.shape[1], _p(off, C.c_int), _p(ids, C.c_int), ncl,
                                        _p(models, C.c_int)), "gpis_ongpis_train")
        return models

    def model(self, slot):
        d = np.zeros(4, dtype=np.int32)
        _check(self.L.gpis_ongpis_model_dims(self.h, int(slot), _p(d, C.c_int)), "gpis_ongpis_model_dims")
        N, ng, K, ld = [int(v) for v in d]
        Lm = np.zeros((ld, ld), dtype=np.float32)
        alpha = np.zeros(K, dtype=np.float32)
        gidx = np.zeros(N, dtype=np.int32)
        _check(self.L.gpis_ongpis_get_model(self.h, int(slot), _p(Lm), _p(alpha), _p(gidx, C.c_int)), "gpis_ongpis_get_model")
        return dict(N=N, ng=ng, K=K, ld=ld, L=Lm.T.copy(), alpha=alpha, gidx=gidx)  # L[r, c]

    def eval(self, xq, job_q, job_model, return_status=False, layout=0):
        """return_status=True: (status, out) instead of raising -- GPIS_ERR_STATE (-3, the kernels' error word) still delivers
        `out`, with the affected results NaN.  layout: 0 every result column, 1 component 0 only, 2 components 1..dim only
        (the other slots of `out` are 0)."""
        xq = np.ascontiguousarray(xq, dtype=np.float32)
        job_q = np.ascontiguousarray(job_q, dtype=np.int32)
        job_model = np.ascontiguousarray(job_model, dtype=np.int32)
        out = np.zeros((job_q.size, 8), dtype=np.float32)
        rc = self.L.gpis_ongpis_eval_layout(self.h, _p(xq), xq.shape[0], _p(job_q, C.c_int), _p(job_model, C.c_int), job_q.size,
                                            int(layout), _p(out))
        if return_status:
            return int(rc), out
        _check(rc, "gpis_ongpis_eval")
        return out

    def packed_bytes(self, models):
        models = np.ascontiguousarray(models, dtype=np.int32)
        return int(self.L.gpis_ongpis_packed_bytes(self.h, _p(models, C.c_int), models.size))

    def pack(self, models, d_buf_ptr, stride, stream=0):
        models = np.ascontiguousarray(models, dtype=np.int32)
        _check(self.L.gpis_ongpis_pack(self.h, _p(models, C.c_int), models.size, C.c_void_p(d_buf_ptr), int(stride), C.c_void_p(stream)),
               "gpis_ongpis_pack")

    def unpack(self, d_buf_ptr, n, stride, models=None, stream=0):
        """records -> predict-only models; returns their ids (new ones unless `models` names slots to reuse)."""
        ids = np.full(n, -1, dtype=np.int32) if models is None else np.ascontiguousarray(models, dtype=np.int32).copy()
        _check(self.L.gpis_ongpis_unpack(self.h, C.c_void_p(d_buf_ptr), int(n), int(stride), _p(ids, C.c_int), C.c_void_p(stream)),
               "gpis_ongpis_unpack")
        return ids

    def kernel_matrix(self, x, gidx, sigx, sigg):
        """Kernel matrix of the build kernel on caller-given arrays (no gather rule): returns K[r, c], lower triangle."""
        x = np.ascontiguousarray(x, dtype=np.float32); gidx = np.ascontiguousarray(gidx, dtype=np.int32)
        sigx = np.ascontiguousarray(sigx, dtype=np.float32); sigg = np.ascontiguousarray(sigg, dtype=np.float32)
        n = gidx.size
        K = n + self.dim * int((gidx >= 0).sum())
        out = np.zeros(K * K, dtype=np.float32)
        _check(self.L.gpis_ongpis_kernel_matrix(self.h, _p(x), _p(gidx, C.c_int), _p(sigx), _p(sigg), n, _p(out)), "gpis_ongpis_kernel_matrix")
        return out.reshape(K, K).T.copy()

    def set_debug(self, inject=0, wait_limit_ms=0):
        """Bound of the in-kernel waits (0 = default 2 s) and the test-only fault injection: inject bit 0 = the cooperative
        factorisation withholds a hand-over, bit 4 (16) = the first workgroup of every prediction launch withholds one ring signal."""
        _check(self.L.gpis_ongpis_set_debug(self.h, int(inject), int(wait_limit_ms)), "gpis_ongpis_set_debug")

    def set_cu_reserve(self, n):
        """CUs the training streams of this handle leave free (CU-masked streams, as the maps' pipelined update uses them)."""
        _check(self.L.gpis_ongpis_set_cu_reserve(self.h, int(n)), "gpis_ongpis_set_cu_reserve")

    def set_lazy_inverse(self, on=True):
        _check(self.L.gpis_ongpis_set_lazy_inverse(self.h, 1 if on else 0), "gpis_ongpis_set_lazy_inverse")

    def set_exp_table(self, on=True):
        _check(self.L.gpis_ongpis_set_exp_table(self.h, 1 if on else 0), "gpis_ongpis_set_exp_table")

    def last_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        self.L.gpis_ongpis_last_ms(self.h, C.byref(a), C.byref(b))
        return a.value, b.value


class MapQueryProbe:
    """Kernel-level K5: the driver of test() (cluster lookup, binning, the evaluation passes, the blend) over the store of an
    OnGPIS handle and a caller-given cluster table.  Test infrastructure: the maps build the same object from their trees."""

    def __init__(self, ongpis, search_half, var_thre, prior_var):
        self.L = lib()
        self.on = ongpis              # (keeps the store alive)
        self.dim = ongpis.dim
        self.h = C.c_void_p(self.L.gpis_mapquery_create(ongpis.h, float(search_half), float(var_thre), float(prior_var)))
        if not self.h:
            raise GpisError("gpis_mapquery_create failed")

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.on, "h", None):
                self.L.gpis_mapquery_destroy(self.h)
            self.h = None

    __del__ = close

    def set_table(self, c, lo, hi, model, parent, anc_lo=None, anc_hi=None, anc_parent=None, pitch=1.0):
        """Entries in traversal order; c / lo / hi [ncl, 3] (third column 0 in 2-D); ancestors parents-first."""
        f32 = lambda a: np.ascontiguousarray(np.zeros((0, 3)) if a is None else a, dtype=np.float32).reshape(-1, 3)
        i32 = lambda a: np.ascontiguousarray(np.zeros(0) if a is None else a, dtype=np.int32).reshape(-1)
        c, lo, hi, anc_lo, anc_hi = f32(c), f32(lo), f32(hi), f32(anc_lo), f32(anc_hi)
        model, parent, anc_parent = i32(model), i32(parent), i32(anc_parent)
        ncl, nanc = c.shape[0], anc_lo.shape[0]
        if not (lo.shape[0] == hi.shape[0] == model.size == parent.size == ncl and anc_hi.shape[0] == anc_parent.size == nanc):
            raise ValueError("set_table: array sizes disagree")
        _check(self.L.gpis_mapquery_set_table(self.h, ncl, _p(c), _p(lo), _p(hi), _p(model, C.c_int), _p(parent, C.c_int), nanc,
                                              _p(anc_lo), _p(anc_hi), _p(anc_parent, C.c_int), float(pitch)), "gpis_mapquery_set_table")

    def set_chunk(self, n):
        _check(self.L.gpis_mapquery_set_chunk(self.h, int(n)), "gpis_mapquery_set_chunk")

    def run(self, x, res):
        """res [n, 2(1+dim)] is input and output: returns a new array, the pre-fill where the reference writes nothing."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.dim)
        res = np.array(res, dtype=np.float32, order="C", copy=True).reshape(x.shape[0], 2 * (1 + self.dim))
        _check(self.L.gpis_mapquery_run(self.h, _p(x), x.shape[0], _p(res)), "gpis_mapquery_run")
        self._n = x.shape[0]
        return res

    def run_device(self, d_x_ptr, n, d_res_ptr, stream=0):
        """run() on the caller's device buffers (raw pointers: x [n, dim], res [n, 2(1+dim)] float32, res input and output), on
        `stream` (0: the store's).  Whatever wrote the buffers must have finished; synchronous on return."""
        _check(self.L.gpis_mapquery_run_device(self.h, C.c_void_p(d_x_ptr), int(n), C.c_void_p(d_res_ptr), C.c_void_p(stream)),
               "gpis_mapquery_run_device")
        self._n = int(n)

    def candidates(self):
        """(ncand [n], cand [3, n]) of the last run (one chunk, non-empty table)."""
        n = getattr(self, "_n", 0)
        ncand = np.zeros(n, dtype=np.int32)
        cand = np.zeros((3, n), dtype=np.int32)
        _check(self.L.gpis_mapquery_candidates(self.h, _p(ncand, C.c_int), _p(cand, C.c_int)), "gpis_mapquery_candidates")
        return ncand, cand

    def pass_jobs(self):
        a = (C.c_longlong * 4)()
        _check(self.L.gpis_mapquery_pass_jobs(self.h, a), "gpis_mapquery_pass_jobs")
        return [int(v) for v in a]

    def set_pass2_mode(self, mode):
        _check(self.L.gpis_mapquery_set_pass2_mode(self.h, int(mode)), "gpis_mapquery_set_pass2_mode")

    def set_k4_schedule(self, mode):
        _check(self.L.gpis_mapquery_set_k4_schedule(self.h, int(mode)), "gpis_mapquery_set_k4_schedule")

    def last_counts(self):
        """Of the last run: last_test_evals, last_test_k4_launches, the queries per chunk, the K4 schedule in force."""
        a = (C.c_longlong * 4)()
        _check(self.L.gpis_mapquery_last_counts(self.h, a), "gpis_mapquery_last_counts")
        return dict(zip(("last_test_evals", "last_test_k4_launches", "chunk", "k4_schedule"), (int(v) for v in a)))

    def pass_detail(self):
        a = (C.c_double * 8)()
        _check(self.L.gpis_mapquery_pass_detail(self.h, a), "gpis_mapquery_pass_detail")
        return dict(zip(GPisMap3.DETAIL_KEYS, list(a)))
