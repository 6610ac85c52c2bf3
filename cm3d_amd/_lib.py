"""Loader of libcm3d_hip.so (the C-ABI declared in include/cm3d_hip.h).

There is no CPU fallback: if the shared library is missing or a symbol cannot
be resolved this raises, and every product entry point fails with it.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CM3D_LIB") or os.path.join(_HERE, "libcm3d_hip.so")      # CM3D_LIB: experiments only

ABI_VERSION = 5
CAM_STRIDE = 64
SWEEP_XF_STRIDE = 24
MAX_CAMS = 8
MAX_MASKS_PER_FRAME = 1024
BOX_STRIDE = 10
MEDOID_TILE = 64
STATUS_WORDS = 4
BBOX_STRIDE = 8          # int32 per mask in `bbox`: eroded bounds [0..3], stored rectangle xw0, y0, wc, rows [4..7] (include/cm3d_hip.h)
MAX_MATCH_BOXES = 1024
MAX_FUSED_SWEEPS = 16
MATCH_BOX_STRIDE = 6
OBB_ROT_STRIDE = 9       # doubles per mask of cm3d_obb's rot_opt (row-major 3x3, ABI v5)
WM_BOX_STRIDE = 8        # doubles per box of cm3d_waymo_metrics
WM_BREAKDOWNS = 16
WM_CUTOFFS = 101
WM_SWEEP_MAX_ALPHAS = 1024   # alphas of one cm3d_waymo_metrics_sweep call
NUSC_MAX_CAND = 1024     # candidates of one group of cm3d_nusc_match
NUSC_MAX_GT = 256        # ground-truth boxes of one group
NUSC_MAX_TH = 4
NUSC_MAX_ALPHAS = 1024   # alphas of one cm3d_nusc_match call
DEPTH_CLUSTER_LDS_POINTS = 4096   # longest list cm3d_depth_cluster sorts in LDS
BEV_FIT_CHUNK = 512      # points of a list cm3d_bev_fit stages in LDS at a time
VERT_LANE_MAX, VERT_LDS_KEYS = 64, 4096      # cm3d_box_vertical: the longest list of the lane route, the most keys staged in LDS
GROUND_BINS = 128        # cm3d_box_ground: the bins of a mask's window
GROUND_GRID_CELLS, GROUND_GRID_BINS = 64, 64      # cm3d_ground_grid: cells per side of a frame's grid, bins of a cell's window
VP_MAX_K, VP_MAX_ROWS, VP_LDS_LIST = 1024, 4096, 256      # cm3d_virtual_points: most points per mask, most image rows, longest list staged in LDS
RAW_QUADS = 3          # raw_stride value of the quad layout (include/cm3d_hip.h, cm3d_sweep_prep)

_p, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); mirrors include/cm3d_hip.h one to one
SIGNATURES = {
    "cm3d_abi_version": (_i32, []),
    "cm3d_project_workgroups_per_cu": (_i32, [_i32]),
    "cm3d_error_string": (C.c_char_p, [_i32]),
    "cm3d_removed_words": (_i64, [_i32, _i32]),
    "cm3d_batch_begin": (_i32, [_p, _p, _i32, _p, _i64, _p]),
    "cm3d_sweep_prep": (_i32, [_p, _i32, _p, _p, _i32, _i32, _p, _p, _i32, _f32, _p, _i32, _p, _p, _p, _p]),
    "cm3d_rle_workspace_bytes": (_i64, [_i32]),
    "cm3d_rle_to_dense": (_i32, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _i64, _p]),
    "cm3d_erode_pack": (_i32, [_p, _i32, _i32, _i32, _p, _p, _p]),
    "cm3d_rle_erode_pack": (_i32, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _i64, _p]),
    "cm3d_rle_erode_pack_begin": (_i32, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _i64, _p, _p, _i32, _p, _i64, _p]),
    "cm3d_rle_erode_pack_sized": (_i32, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _i64, _p]),
    "cm3d_rle_erode_pack_sized_begin": (_i32, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _i64, _p, _p, _i32, _p, _i64, _p]),
    "cm3d_project_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "cm3d_project_hit_rows": (_i32, [_p, _i64, _i32, _i32, _i32, _p, _p]),
    "cm3d_project_culling": (_i32, [_p, _i64, _i32, _i32, _i32, _p, _p]),
    "cm3d_project_wedges": (_i32, [_p, _i64, _i32, _i32, _i32, _p, _p]),
    "cm3d_project_hits": (_i32, [_p, _p, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _p, _i32, _i32, _i32, _f32, _i32,
                                 _p, _p, _p, _p, _i64, _p, _p, _p]),
    "cm3d_sweep_project_hits": (_i32, [_p, _i32, _p, _p, _i32, _i32, _p, _p, _f32, _p, _i32, _p, _p, _i32, _i32, _i32, _p, _i32, _p, _p,
                                       _p, _p, _i32, _i32, _i32, _f32, _i32, _p, _p, _p, _p, _i64, _p, _p, _p]),
    "cm3d_compact_hits": (_i32, [_p, _i32, _i32, _i32, _i32, _p, _i32, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p,
                                 _i64, _p]),
    "cm3d_tile_work_bytes": (_i64, [_i32, _i32]),
    "cm3d_selftest_sqrt": (_i32, [C.c_uint32, C.c_uint32, _p, _p, _p]),
    "cm3d_selftest_div": (_i32, [C.c_uint64, C.c_uint64, _p, _p]),
    "cm3d_selftest_mfma": (_i32, [C.c_uint64, _i32, _p, _p]),
    "cm3d_medoid_workspace_bytes": (_i64, [_i32, _i32]),
    "cm3d_medoid": (_i32, [_p, _p, _p, _i32, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_medoid2": (_i32, [_p, _p, _p, _i32, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _i64, _i32, _p, _p]),
    "cm3d_lane_grid_bytes": (_i64, [_i32, _i32]),
    "cm3d_lane_grid_build": (_i32, [_p, _p, _i32, _i32, _p, _i64, _p]),
    "cm3d_lane_nn_workspace_bytes": (_i64, [_i32]),
    "cm3d_lane_nn": (_i32, [_p, _p, _p, _i32, _p, _p, _p, _i32, _i32, _p, _p, _p, _p, _i64, _p]),
    "cm3d_circle_nms": (_i32, [_p, _p, _p, _p, _p, _i32, _p, _i32, _p, _p]),
    "cm3d_rotated_nms": (_i32, [_p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p]),
    "cm3d_box_rotated_nms": (_i32, [_p, _p, _p, _i32, _i32, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _i32, _i32, _p]),
    "cm3d_box_nms": (_i32, [_p, _p, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p, _p, _p]),
    "cm3d_box_nms_bounded": (_i32, [_p, _p, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _i32, _p, _p, _p]),
    "cm3d_centroid_transform": (_i32, [_p, _p, _p, _i32, _p, _p, _p]),
    "cm3d_bev_match_workspace_bytes": (_i64, [_i64]),
    "cm3d_bev_match": (_i32, [_p, _p, _i32, _p, _p, _i32, _p, _i32, _i64, C.c_double, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_obb_workspace_bytes": (_i64, [_i32, _i32]),
    "cm3d_obb": (_i32, [_p, _p, _i32, _i32, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_selftest_obb_yaw": (_i32, [_p, _i32, _p, _p]),
    "cm3d_waymo_metrics_workspace_bytes": (_i64, [_i64]),
    "cm3d_waymo_metrics": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _p, _p, _p, _p, _i64, _p]),
    "cm3d_waymo_metrics_sweep_workspace_bytes": (_i64, [_i64]),
    "cm3d_waymo_metrics_sweep": (_i32, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _i64, _p, _i32, _p, _p, _p, _p, _i64, _p]),
    "cm3d_nusc_match_workspace_bytes": (_i64, [_i32, _i64, _i32]),
    "cm3d_nusc_match": (_i32, [_p, _p, _p, _p, _p, _p, _p, _i32, _i64, _p, _i32, _p, _i32, _p, _p, _p, _p, _i64, _p]),
    "cm3d_lift_pass": (_i32, [_p, _p]),
    "cm3d_pipe_exec_streams_for": (_i32, [_i32, _i32]),
    "cm3d_pipe_create": (_p, [_i32, _i32, _p]),
    "cm3d_pipe_create2": (_p, [_i32, _i32, _p, _i32]),
    "cm3d_pipe_null_exec": (_i32, [_p]),
    "cm3d_pipe_destroy": (None, [_p]),
    "cm3d_pipe_exec_streams": (_i32, [_p]),
    "cm3d_pipe_submit": (_i32, [_p, _i32, _p]),
    "cm3d_pipe_acquire": (_i32, [_p, _i32]),
    "cm3d_pipe_release": (_i32, [_p, _i32]),
    "cm3d_pipe_wait": (_i32, [_p, _i32]),
    "cm3d_pipe_pin": (_i32, [_p]),
    "cm3d_pipe_last_stream": (_i32, [_p, _i32]),
    "cm3d_points_in_polygons": (_i32, [_p, _p, _i32, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p]),
    "cm3d_stage2_filter": (_i32, [_p, _p, _p, _p, _p, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _i32, C.c_double, C.c_double,
                                  _p, _p, _p]),
    "cm3d_lift_pass_filtered": (_i32, [_p, _p, _p]),
    "cm3d_lift_pass_head": (_i32, [_p, _p]),
    "cm3d_lift_pass_tail": (_i32, [_p, _p]),
    "cm3d_depth_cluster_workspace_bytes": (_i64, [_i32, _i32]),
    "cm3d_depth_cluster": (_i32, [_p, _p, _p, _p, _i32, _i32, _p, _i32, C.c_double, _i32, _i32, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_lift_pass_clustered": (_i32, [_p, _p, _p]),
    "cm3d_bev_fit": (_i32, [_p, _p, _i32, _i32, _p, _i32, C.c_double, _i32, C.c_double, _p, _p, _p, _p]),
    "cm3d_yaw_select": (_i32, [_p, _p, _p, _p, _p, _p, _i32, _p, C.c_double, _p, _p, _p, _p, _i32, _i32, _p, _i32, _i32, _p, _p, _p, _p]),
    "cm3d_yaw_fit_boxes": (_i32, [_p, _p, _p]),
    "cm3d_lift_pass_yaw_fitted": (_i32, [_p, _p, _p]),
    "cm3d_lift_pass_opt": (_i32, [_p, _p, _p]),
    "cm3d_box_velocity_workspace_bytes": (_i64, [_i64, _i32]),
    "cm3d_box_velocity": (_i32, [_p, _p, _p, _i32, _i32, _p, _p, _p, _i32, _i32, _p, _p, C.c_double, _p, _i32, _i64, _p, _p, _p, _p, _p, _p,
                                 _i64, _p]),
    "cm3d_box_tracks_workspace_bytes": (_i64, [_i32]),
    "cm3d_box_tracks": (_i32, [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_box_place": (_i32, [_p, _p, _p, _i32, _i32, _p, _p, _p, _p, _p, _i32, _p, _i32, C.c_double, _i32, _p, _p, _p]),
    "cm3d_lift_pass_placed": (_i32, [_p, _p, _p, _p]),
    "cm3d_box_size_workspace_bytes": (_i64, [_i32]),
    "cm3d_box_size": (_i32, [_p, _p, _p, _p, _p, _p, _i32, _p, _i32, C.c_double, _p, _p, _p, _p, _p, _p, _i32, _i32, C.c_double, _i32,
                             C.c_double, _i32, C.c_double, C.c_double, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_box_vertical": (_i32, [_p, _p, _i32, _i32, _p, _p, _p, _i32, C.c_double, C.c_double, _i32, C.c_double, C.c_double, _p, _p, _p,
                                 _p, _p, _p]),
    "cm3d_box_ground_chunk": (_i32, [_i32, _i32]),
    "cm3d_box_ground": (_i32, [_p, _p, _p, _i32, _p, _p, _p, _i32, _f32, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _i32, _p, _p, _p, _p,
                               C.c_double, C.c_double, _i32, C.c_double, C.c_double, C.c_double, C.c_double, _p, _p, _p, _p, _p, _p, _p]),
    "cm3d_ground_strip_check": (_i32, [C.c_double, C.c_double, C.c_double, C.c_double, _i32, C.c_double, _i32]),
    "cm3d_ground_grid": (_i32, [_p, _p, _p, _i32, _p, _p, _p, _i32, _f32, _i32, _p, _i32, C.c_double, C.c_double, C.c_double, C.c_double,
                                _i32, _p, _p, _p]),
    "cm3d_ground_strip_workspace_bytes": (_i64, [_i32, _i32]),
    "cm3d_ground_strip": (_i32, [_p, _p, _p, _p, _i32, _i32, _p, _p, _i32, C.c_double, C.c_double, _i32, _p, _p, _p, _p, _p, _p, _p, _i64,
                                 _p]),
    "cm3d_lift_pass_stripped": (_i32, [_p, _p, _p, _p, _p]),
    "cm3d_virtual_points_check": (_i32, [_i32, C.c_double]),
    "cm3d_hit_project": (_i32, [_p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "cm3d_virtual_points": (_i32, [_p, _p, _i32, _i32, _p, _i32, _p, _p, _p, _p, _i32, _i32, _p, _p, _i32, _i32, C.c_uint32, C.c_double, _i32,
                                   _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "cm3d_point_owner_check": (_i32, [_i32, _i32]),
    "cm3d_point_owner_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "cm3d_point_owner": (_i32, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "cm3d_lift_pass_owned": (_i32, [_p, _p, _p, _p, _p, _p]),
    "cm3d_lift_pass_composed": (_i32, [_p, _p, _p, _p, _p, _p]),
}

POLY_INDEX_ARRAYS = ("tab_y", "tab_slab", "slab_off", "ent_edge", "ent_ring", "edge", "ring_info")     # cm3d_points_in_polygons, in order


class LiftPassDesc(C.Structure):
    """cm3d_lift_pass_desc of include/cm3d_hip.h, field for field."""
    _fields_ = (
        [("size", _i64)]
        + [(n, _p) for n in ("rle_counts", "rle_off", "packed", "bbox", "rle_ws")] + [("rle_ws_bytes", _i64)]
        + [(n, _p) for n in ("status", "hit_count", "removed_bits")] + [("removed_words", _i64)]
        + [(n, _p) for n in ("raw", "intensity", "sweep_row_off", "sweep_xf", "frame_sweep_off", "points", "pt_off", "cams", "mask_off",
                             "mask_cam", "hit_words", "pg_ws")] + [("pg_ws_bytes", _i64)]
        + [(n, _p) for n in ("hit_off", "tile_off", "hit_idx", "hit_xyz", "tile_work", "medoid_pos", "centroid", "colsum", "ws")]
        + [("ws_bytes", _i64), ("md_feedback", _p)]
        + [(n, _p) for n in ("centroid_g", "mask_frame", "lane", "lane_off", "frame_lane", "grid", "lane_idx", "lane_dist", "class_id", "score",
                             "prior_wlh", "is_vehicle", "nms_group", "nms_thr", "ego_xyz", "box", "flags")]
        + [(n, _p) for n in ("mask_wh", "pose_rt", "pose_inv", "obb_yaw", "obb_status", "obb_ws")] + [("obb_ws_bytes", _i64)]
        + [("dense", _p), ("lane_ready", _p), ("ev_project", _p * 2), ("ev_stage", _p * 5)]
        + [(n, _i32) for n in ("n_masks", "total_runs", "W", "H", "raw_stride", "n_sweeps", "max_sweeps_per_frame", "max_rows_per_sweep",
                               "pt_cap", "n_frames", "max_pts_per_frame", "n_cams", "planes", "idx_cap", "n_tables", "n_lane_points",
                               "n_classes")]
        + [("halfw", _f32), ("min_dist", _f32)]
        + [(n, _i32) for n in ("md_hint", "fused", "separate_reset")])


class Stage2FilterDesc(C.Structure):
    """cm3d_stage2_filter_desc of include/cm3d_hip.h, field for field."""
    _fields_ = ([("size", _i64)] + [(n, _p) for n in POLY_INDEX_ARRAYS + ("needs_road", "medoid_pos_kept", "on_road")]
                + [("ev", _p * 2), ("lane_max_dist", C.c_double), ("vehicle_lane_max_dist", C.c_double), ("n_poly_tables", _i32),
                   ("reserved", _i32)])


class DepthClusterDesc(C.Structure):
    """cm3d_depth_cluster_desc of include/cm3d_hip.h, field for field."""
    _fields_ = ([("size", _i64)] + [(n, _p) for n in ("origin", "cl_off", "cl_tile_off", "cl_idx", "cl_xyz", "cl_status", "ws")]
                + [("ws_bytes", _i64), ("ev", _p * 2), ("eps", C.c_double), ("min_points", _i32), ("pick", _i32)])


class YawFitDesc(C.Structure):
    """cm3d_yaw_fit_desc of include/cm3d_hip.h, field for field."""
    _fields_ = ([("size", _i64)] + [(n, _p) for n in ("angle_cs", "hit_xyz", "hit_off", "medoid_pos", "fit_k", "fit_rect", "fit_status",
                                                      "yaw_tab", "yaw_idx", "yaw_src", "tab_off", "tab_frame")]
                + [("ev", _p * 2), ("d0", C.c_double), ("min_length", C.c_double), ("lane_min_dist", C.c_double), ("K", _i32),
                   ("min_points", _i32)])


class RotatedNmsDesc(C.Structure):
    """cm3d_rotated_nms_desc of include/cm3d_hip.h, field for field."""
    _fields_ = [("size", _i64), ("thr", _p), ("n_thr", _i32), ("measure", _i32), ("class_agnostic", _i32), ("reserved", _i32)]


class LiftPassOptions(C.Structure):
    """cm3d_lift_pass_options of include/cm3d_hip.h, field for field: pointers to the descriptors above, NULL for a stage that is off."""
    _fields_ = [("size", _i64)] + [(n, _p) for n in ("cluster", "filter", "yaw", "nms")]


class BoxPlaceDesc(C.Structure):
    """cm3d_box_place_desc of include/cm3d_hip.h, field for field."""
    _fields_ = [("size", _i64), ("place_src", _p), ("place_pushed", _p), ("ev", _p * 2), ("thin", C.c_double)]


class GroundStripDesc(C.Structure):
    """cm3d_ground_strip_desc of include/cm3d_hip.h, field for field."""
    _fields_ = ([("size", _i64)] + [(n, _p) for n in ("origin", "grid_z", "grid_n", "gs_off", "gs_tile_off", "gs_idx", "gs_xyz", "gs_status",
                                                      "gs_dropped", "ws")]
                + [("ws_bytes", _i64), ("ev", _p * 2)] + [(n, C.c_double) for n in ("cell", "down", "up", "quantile", "margin")]
                + [("min_points", _i32), ("min_keep", _i32)])


class PointOwnerDesc(C.Structure):
    """cm3d_point_owner_desc of include/cm3d_hip.h, field for field."""
    _fields_ = ([("size", _i64)] + [(n, _p) for n in ("ow_owner", "ow_off", "ow_tile_off", "ow_idx", "ow_xyz", "ow_status", "ow_lost", "ws")]
                + [("ws_bytes", _i64), ("ev", _p * 2), ("rule", _i32), ("min_keep", _i32)])


class Cm3dError(RuntimeError):
    pass


_lib = None


def lib():
    """The loaded library (loads on first use).  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Cm3dError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the lifting path.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)       # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.cm3d_abi_version() != ABI_VERSION:
            raise Cm3dError("libcm3d_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().cm3d_error_string(code).decode()
        raise Cm3dError(f"{what}: {msg} ({code})")
