"""ctypes binding of librsm_mi355.so (include/rsm.h).

There is no CPU fallback: if the HIP library is missing or no MI355X is visible the product path
raises -- it never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librsm_mi355.so")

RSM_OK = 0
RSM_E_INVALID = -1
RSM_E_DEGENERATE_MARGIN = -2
RSM_E_HIP = -3
RSM_E_NOMEM = -4
RSM_E_STATE = -5
RSM_E_COMM = -6
RSM_W_NOT_CONVERGED = 1   # rsm_poisson_mesh / rsm_stage_poisson_solve: max_cycles reached; the results are valid
NOMATCH = -10000


class RsmError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("rsm error %d: %s" % (code, msg))
        self.code = code


class Boundary(C.Structure):
    """struct Boundary (CManageData.h:10-14)."""
    _fields_ = [("YL", C.c_int), ("YR", C.c_int), ("XL", C.c_int), ("XR", C.c_int),
                ("width", C.c_int), ("height", C.c_int)]

    def astuple(self):
        return (self.YL, self.YR, self.XL, self.XR, self.width, self.height)

    def __repr__(self):
        return "Boundary(YL=%d,YR=%d,XL=%d,XR=%d,w=%d,h=%d)" % self.astuple()


class PairIn(C.Structure):
    _fields_ = [("image", C.c_void_p * 2), ("mask", C.c_void_p * 2),
                ("width", C.c_int), ("height", C.c_int), ("pyr_levels", C.c_int),
                ("radius", C.c_int), ("ws", C.c_double), ("offset", C.c_int),
                ("origin_width", C.c_int), ("Q", C.c_double * 16), ("R_final", C.c_double * 9),
                ("T_final", C.c_double * 3), ("verbose", C.c_int)]


RSM_ABI_VERSION = 2   # include/rsm.h: the struct layouts mirrored here (PairOut carries points16); load() holds the library to it


class PairOut(C.Structure):
    _fields_ = [("disparity", C.c_void_p * 2), ("margin", Boundary * 2),
                ("n_points", C.c_int64), ("max_points", C.c_int64),
                ("xyz", C.c_void_p), ("bgr", C.c_void_p), ("v_top", C.c_int64), ("points16", C.c_void_p)]


class FilterParams(C.Structure):
    _fields_ = [("sor_mean_k", C.c_int), ("sor_std_mul", C.c_double), ("normal_radius", C.c_double), ("cam_center", C.c_float * 3)]


class OutremParams(C.Structure):
    """rsm_outrem_params (include/rsm.h)."""
    _fields_ = [("min_neighbors", C.c_int), ("radius", C.c_double)]


class MlsParams(C.Structure):
    """rsm_mls_params (include/rsm.h)."""
    _fields_ = [("search_radius", C.c_double), ("polynomial_order", C.c_int)]


class PoissonParams(C.Structure):
    """rsm_poisson_params (include/rsm.h)."""
    _fields_ = [("depth", C.c_int), ("scale", C.c_double), ("rel_residual", C.c_double), ("max_cycles", C.c_int), ("trim_cells", C.c_int)]


POISSON_STATS = 12


class PoissonDensityParams(C.Structure):
    """rsm_poisson_density_params (include/rsm.h)."""
    _fields_ = [("kernel_depth", C.c_int), ("samples_per_node", C.c_double)]


POISSON_WEIGHTED_STATS = 16


class PoissonBandParams(C.Structure):
    """rsm_poisson_band_params (include/rsm.h)."""
    _fields_ = [("band_bricks", C.c_int), ("max_iterations", C.c_int)]


POISSON_BAND_STATS = 17
POISSON_BAND_MAX_BRICKS = 1 << 20
POISSON_BAND_WEIGHTED_STATS = 21   # RSM_POISSON_BAND_WEIGHTED_STATS


class MeshCleanParams(C.Structure):
    """rsm_mesh_clean_params (include/rsm.h)."""
    _fields_ = [("smooth_steps", C.c_int), ("cotangent", C.c_int), ("boundary", C.c_int), ("min_piece", C.c_double),
                ("min_piece_relative", C.c_int), ("flags", C.c_uint)]


MESH_CLEAN_STATS = 14
MESH_CLEAN_DUPLICATES, MESH_CLEAN_ZERO_AREA, MESH_CLEAN_NONMANIFOLD = 1, 2, 4


class MeshTrimParams(C.Structure):
    """rsm_mesh_trim_params (include/rsm.h)."""
    _fields_ = [("depth", C.c_int), ("scale", C.c_double), ("kernel_depth", C.c_int), ("samples_per_node", C.c_double), ("smooth_steps", C.c_int),
                ("trim", C.c_double), ("island_ratio", C.c_double)]


MESH_TRIM_STATS = 20


class MeshCloseParams(C.Structure):
    """rsm_mesh_close_params (include/rsm.h)."""
    _fields_ = [("max_hole_size", C.c_int)]


MESH_CLOSE_STATS = 14
MESH_CLOSE_MAX_HOLE = 64


class MeshDecimateParams(C.Structure):
    """rsm_mesh_decimate_params (include/rsm.h)."""
    _fields_ = [("target_faces", C.c_int64), ("target_fraction", C.c_double), ("quality_thr", C.c_double), ("preserve_boundary", C.c_int),
                ("boundary_weight", C.c_double), ("preserve_normal", C.c_int), ("preserve_topology", C.c_int), ("optimal_placement", C.c_int),
                ("min_error", C.c_double), ("max_rounds", C.c_int)]


MESH_DECIMATE_STATS = 20


class MeshSubdivideParams(C.Structure):
    """rsm_mesh_subdivide_params (include/rsm.h)."""
    _fields_ = [("iterations", C.c_int), ("threshold", C.c_double), ("threshold_fraction", C.c_double), ("weight_scheme", C.c_int)]


MESH_SUBDIVIDE_STATS = 17


class MeshColorParams(C.Structure):
    """rsm_mesh_color_params (include/rsm.h)."""
    _fields_ = [("mode", C.c_int), ("min_cos", C.c_double), ("depth_eps", C.c_double)]


MESH_COLOR_STATS = 6


class MeshStitchParams(C.Structure):
    """rsm_mesh_stitch_params (include/rsm.h); `lambda` is set by position or setattr."""
    _fields_ = [("lambda", C.c_double), ("iterations", C.c_int), ("reduction", C.c_double), ("seam_gradient", C.c_int)]


MESH_STITCH_STATS = 12


class MeshFillParams(C.Structure):
    """rsm_mesh_fill_params (include/rsm.h)."""
    _fields_ = [("max_rounds", C.c_int), ("iterations", C.c_int), ("reduction", C.c_double)]


MESH_FILL_STATS = 10


class DedupView(C.Structure):
    """rsm_dedup_view (include/rsm.h): one pair of the rig for the duplicate deletion (host pointers)."""
    _fields_ = [("P", (C.c_double * 12) * 2), ("cam_center", C.c_float * 3), ("bound0", Boundary), ("width", C.c_int),
                ("height", C.c_int), ("image", C.c_void_p * 2), ("mask", C.c_void_p * 2)]


class RectifyIn(C.Structure):
    _fields_ = [("K", (C.c_double * 9) * 2), ("E", (C.c_double * 12) * 2),
                ("origin_width", C.c_int), ("origin_height", C.c_int), ("lowest_width", C.c_int),
                ("lowest_height", C.c_int), ("pyr_levels", C.c_int),
                ("image", C.c_void_p * 2), ("mask", C.c_void_p * 2)]


class RectifyOut(C.Structure):
    _fields_ = [("Q", C.c_double * 16), ("R_final", C.c_double * 9), ("T_final", C.c_double * 3),
                ("P", (C.c_double * 12) * 2), ("width", C.c_int), ("height", C.c_int),
                ("image", C.c_void_p * 2), ("mask", C.c_void_p * 2)]


# ---- the prototypes of include/rsm.h, one row per function: name -> (restype, argtypes); tests/test_abi.py holds every row against the header.
# Pointers to the structs above are typed; every other data, handle or array pointer is void *.
_I, _L, _U, _LL, _Z, _D, _V, _S = C.c_int, C.c_int64, C.c_uint32, C.c_longlong, C.c_size_t, C.c_double, C.c_void_p, C.c_char_p
_pI, _pL, _pD = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
_PIN, _POUT, _BND, _RIN, _ROUT, _FLT = (C.POINTER(t) for t in (PairIn, PairOut, Boundary, RectifyIn, RectifyOut, FilterParams))
_MLS, _VIEW, _PSN, _CLN, _COL, _STI = (C.POINTER(t) for t in (MlsParams, DedupView, PoissonParams, MeshCleanParams, MeshColorParams, MeshStitchParams))
_TRM, _CLO, _DEC, _PDN = C.POINTER(MeshTrimParams), C.POINTER(MeshCloseParams), C.POINTER(MeshDecimateParams), C.POINTER(PoissonDensityParams)
_SUB, _PBD, _FIL = C.POINTER(MeshSubdivideParams), C.POINTER(PoissonBandParams), C.POINTER(MeshFillParams)
_ORM = C.POINTER(OutremParams)
PROTOTYPES = {
    "rsm_create": (_I, [_V, _I]),
    "rsm_destroy": (None, [_V]),
    "rsm_last_error": (_S, [_V]),
    "rsm_version": (_S, []),
    "rsm_abi_version": (_I, []),
    "rsm_device_count": (_I, []),
    "rsm_match_pair": (_I, [_V, _PIN, _POUT]),
    "rsm_upload_pair": (_I, [_V, _PIN]),
    "rsm_upload_pair_device": (_I, [_V, _PIN]),
    "rsm_run_pair": (_I, [_V]),
    "rsm_download_pair": (_I, [_V, _POUT]),
    "rsm_host_alloc": (_V, [_Z]),
    "rsm_host_free": (None, [_V]),
    "rsm_host_register": (_I, [_V, _Z]),
    "rsm_host_unregister": (_I, [_V]),
    "rsm_result_device": (_I, [_V, _V, _V, _V, _V, _V]),
    "rsm_export_cloud_device": (_I, [_V, _V, _V, _L]),
    "rsm_run_pairs": (_I, [_V, _I]),
    "rsm_run_pairs_repeat": (_I, [_V, _I, _I]),
    "rsm_match_pairs": (_I, [_V, _I, _PIN, _POUT, _I, _V]),
    "rsm_match_pairs_multi_gpu": (_I, [_PIN, _I, _I, _I, _POUT, _V]),
    "rsm_pack_cloud16": (_I, [_V, _V, _L, _V]),
    "rsm_comm_unique_id": (_I, [_S]),
    "rsm_comm_create": (_I, [_V, _S, _I, _I, _I]),
    "rsm_comm_create_transport": (_I, [_V, _V, _I, _I]),
    "rsm_comm_destroy": (None, [_V]),
    "rsm_comm_last_error": (_S, [_V]),
    "rsm_gather_clouds": (_I, [_V, _I, _I, _V, _V, _V, _I, _V, _L, _V]),
    "rsm_gather_counts": (_I, [_V, _I, _V, _V, _I, _V]),
    "rsm_gather_meta_fill": (_I, [_I, _I, _I, _I, _V, _V, _I, _L, _V]),
    "rsm_gather_plan": (_I, [_I, _I, _I, _I, _V, _V, _I, _V, _V, _V, _I, _V]),
    "rsm_set_option": (_I, [_V, _S, _LL]),
    "rsm_profile_enable": (_I, [_V, _I]),
    "rsm_profile_stage_count": (_I, []),
    "rsm_profile_stage_name": (_S, [_I]),
    "rsm_profile_get": (_I, [_V, _V, _V, _V]),
    "rsm_stage_find_margin": (_I, [_V, _V, _I, _I, _I, _BND]),
    "rsm_stage_pyr_down": (_I, [_V, _V, _I, _I, _I, _V]),
    "rsm_stage_erode_ellipse": (_I, [_V, _V, _I, _I, _I, _V]),
    "rsm_stage_box_sums": (_I, [_V, _V, _I, _I, _I, _V, _V]),
    "rsm_stage_initial_match": (_I, [_V, _V, _V, _V, _V, _I, _I, _I, _I, _BND, _BND, _V, _I, _I, _V]),
    "rsm_stage_last_ncc_routes": (_I, [_V, _I, _V, _V, _V, _V, _V, _V]),
    "rsm_stage_smooth": (_I, [_V, _V, _I, _I, _BND]),
    "rsm_stage_order": (_I, [_V, _V, _I, _I, _BND]),
    "rsm_stage_uniqueness_pass_s16": (_I, [_V, _V, _V, _I, _I, _BND, _BND]),
    "rsm_stage_uniqueness_pass_f64": (_I, [_V, _V, _V, _I, _I, _BND, _BND]),
    "rsm_stage_set_boundary": (_I, [_V, _V, _V, _I, _I, _BND, _BND, _V, _V]),
    "rsm_stage_rematch": (_I, [_V, _V, _V, _V, _V, _I, _I, _I, _BND, _BND, _V]),
    "rsm_stage_median": (_I, [_V, _V, _V, _I, _I, _BND]),
    "rsm_stage_refine": (_I, [_V, _V, _V, _V, _I, _I, _I, _D, _BND, _V]),
    "rsm_stage_exp_neg": (_I, [_V, _V, _L, _V]),
    "rsm_stage_exp_neg_small": (_I, [_V, _V, _L, _V]),
    "rsm_stage_div_unscaled": (_I, [_V, _V, _V, _L, _V, _V]),
    "rsm_stage_sqrt_check": (_I, [_V, _U, _L, _V]),
    "rsm_stage_win_index_check": (_I, [_V, _I, _I, _V]),
    "rsm_stage_refine_xi": (_I, [_V, _V, _V, _I, _I, _I, _V]),
    "rsm_stage_cloud": (_I, [_V, _V, _V, _V, _I, _I, _V, _D, _V, _V, _BND, _V, _V, _L, _V]),
    "rsm_rectify_pair": (_I, [_V, _RIN, _I, _D, _I, _I, _ROUT]),
    "rsm_stereo_rectify": (_I, [_V, _V, _I, _I, _V, _V, _V, _V, _V, _V, _V]),
    "rsm_stage_rect_map": (_I, [_V, _V, _V, _V, _I, _I, _V, _V]),
    "rsm_stage_remap": (_I, [_V, _V, _I, _I, _I, _V, _V, _I, _I, _V]),
    "rsm_stage_erode_gray": (_I, [_V, _V, _I, _I, _I, _V]),
    "rsm_write_ply": (_I, [_S, _V, _V, _L]),
    "rsm_write_ply16": (_I, [_S, _V, _L]),
    "rsm_filter_cloud": (_I, [_V, _V, _L, _FLT, _V, _V, _V, _V]),
    "rsm_filter_last_cloud": (_I, [_V, _FLT, _V, _V, _L, _V, _V]),
    "rsm_filter_last_info": (_I, [_V, _V]),
    "rsm_filter_last_normals_info": (_I, [_V, _V]),
    "rsm_filter_last_grid": (_I, [_V, _V, _V]),
    "rsm_filter_last_passes": (_I, [_V, _V, _V, _L, _V]),
    "rsm_stage_filter_depth_map": (_I, [_V, _V, _V, _V, _I, _I, _V, _D, _V, _V, _BND, _FLT, _V, _V, _V, _L, _V, _V, _V]),
    "rsm_filter_last_cloud_host": (_I, [_V, _FLT, _V, _V, _L, _V, _V]),
    "rsm_filter_set_outrem": (_I, [_V, _ORM]),
    "rsm_filter_last_outrem": (_I, [_V, _V]),
    "rsm_stage_radius_count": (_I, [_V, _V, _L, _D, _I, _V]),
    "rsm_mls_cloud": (_I, [_V, _V, _L, _V, _MLS, _V, _V, _V, _pL]),
    "rsm_mls_cloud_device": (_I, [_V, _V, _L, _V, _MLS, _V, _V, _V, _pL]),
    "rsm_dedup_cloud": (_I, [_V, _V, _V, _L, _VIEW, _I, _V, _pL, _pL]),
    "rsm_dedup_cloud_device": (_I, [_V, _V, _V, _L, _VIEW, _I, _V, _V, _V, _pL, _pL]),
    "rsm_poisson_mesh": (_I, [_V, _V, _V, _L, _PSN, _pL, _pL, _V]),
    "rsm_poisson_mesh_device": (_I, [_V, _V, _V, _L, _PSN, _pL, _pL, _V]),
    "rsm_poisson_last_mesh": (_I, [_V, _V, _V]),
    "rsm_poisson_last_mesh_device": (_I, [_V, _V, _V]),
    "rsm_stage_poisson_rhs": (_I, [_V, _V, _V, _L, _PSN, _V, _V, _V, _V]),
    "rsm_stage_poisson_solve": (_I, [_V, _V, _I, _D, _I, _V, _pD, _pI, _V]),
    "rsm_stage_iso_mesh": (_I, [_V, _V, _I, _D, _V, _V, _I, _pL, _pL]),
    "rsm_poisson_mesh_weighted": (_I, [_V, _V, _V, _L, _PSN, _PDN, _pL, _pL, _V]),
    "rsm_poisson_mesh_weighted_device": (_I, [_V, _V, _V, _L, _PSN, _PDN, _pL, _pL, _V]),
    "rsm_stage_poisson_rhs_weighted": (_I, [_V, _V, _V, _L, _PSN, _PDN, _V, _V, _V, _V, _V, _V, _V, _V]),
    "rsm_poisson_mesh_banded": (_I, [_V, _V, _V, _L, _PSN, _PBD, _pL, _pL, _V]),
    "rsm_poisson_mesh_banded_device": (_I, [_V, _V, _V, _L, _PSN, _PBD, _pL, _pL, _V]),
    "rsm_stage_poisson_band_rhs": (_I, [_V, _V, _V, _L, _PSN, _PBD, _V, _L, _L, _V, _V, _V, _V, _V, _V]),
    "rsm_poisson_mesh_banded_weighted": (_I, [_V, _V, _V, _L, _PSN, _PBD, _PDN, _pL, _pL, _V]),
    "rsm_poisson_mesh_banded_weighted_device": (_I, [_V, _V, _V, _L, _PSN, _PBD, _PDN, _pL, _pL, _V]),
    "rsm_stage_poisson_band_rhs_weighted": (_I, [_V, _V, _V, _L, _PSN, _PBD, _PDN, _V, _V, _L, _L, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "rsm_stage_poisson_band_solve": (_I, [_V, _V, _L, _I, _V, _V, _V, _D, _I, _V, _pD, _pI, _pD, _V]),
    "rsm_stage_band_iso_mesh": (_I, [_V, _V, _L, _I, _V, _D, _V, _V, _I, _pL, _pL]),
    "rsm_write_ply_mesh": (_I, [_S, _V, _L, _V, _L]),
    "rsm_mesh_clean": (_I, [_V, _V, _L, _V, _L, _CLN, _pL, _pL, _V]),
    "rsm_mesh_clean_device": (_I, [_V, _V, _L, _V, _L, _CLN, _pL, _pL, _V]),
    "rsm_mesh_clean_last": (_I, [_V, _CLN, _pL, _pL, _V]),
    "rsm_stage_mesh_smooth": (_I, [_V, _V, _L, _V, _L, _I, _I, _I, _V, _pL]),
    "rsm_stage_mesh_components": (_I, [_V, _V, _L, _L, _V, _pL]),
    "rsm_mesh_trim": (_I, [_V, _V, _L, _V, _L, _V, _V, _L, _TRM, _pL, _pL, _V]),
    "rsm_mesh_trim_device": (_I, [_V, _V, _L, _V, _L, _V, _V, _L, _TRM, _pL, _pL, _V]),
    "rsm_mesh_trim_last": (_I, [_V, _V, _V, _L, _TRM, _pL, _pL, _V]),
    "rsm_stage_mesh_density": (_I, [_V, _V, _V, _L, _TRM, _V, _L, _V, _V, _V]),
    "rsm_stage_mesh_value_smooth": (_I, [_V, _V, _L, _L, _V, _I, _V]),
    "rsm_stage_mesh_split": (_I, [_V, _V, _L, _V, _L, _V, _D, _D, _pL, _pL, _V, _V, _V, _V]),
    "rsm_mesh_close_holes": (_I, [_V, _V, _L, _V, _L, _CLO, _pL, _pL, _V]),
    "rsm_mesh_close_holes_device": (_I, [_V, _V, _L, _V, _L, _CLO, _pL, _pL, _V]),
    "rsm_mesh_close_holes_last": (_I, [_V, _CLO, _pL, _pL, _V]),
    "rsm_stage_mesh_border_loops": (_I, [_V, _V, _L, _L, _V, _V, _pL]),
    "rsm_stage_hole_triangulate": (_I, [_V, _V, _I, _V, _pD, _V, _pI]),
    "rsm_mesh_decimate": (_I, [_V, _V, _L, _V, _L, _DEC, _pL, _pL, _V]),
    "rsm_mesh_decimate_device": (_I, [_V, _V, _L, _V, _L, _DEC, _pL, _pL, _V]),
    "rsm_mesh_decimate_last": (_I, [_V, _DEC, _pL, _pL, _V]),
    "rsm_stage_mesh_quadrics": (_I, [_V, _V, _L, _V, _L, _D, _V]),
    "rsm_stage_mesh_collapse_costs": (_I, [_V, _V, _L, _V, _L, _V, _DEC, _V, _V, _V, _V, _V, _pL]),
    "rsm_stage_mesh_collapse_round": (_I, [_V, _V, _L, _V, _L, _V, _DEC, _L, _V, _V, _V, _pL, _V, _pL, _pL]),
    "rsm_mesh_subdivide": (_I, [_V, _V, _L, _V, _L, _SUB, _pL, _pL, _V]),
    "rsm_mesh_subdivide_device": (_I, [_V, _V, _L, _V, _L, _SUB, _pL, _pL, _V]),
    "rsm_mesh_subdivide_last": (_I, [_V, _SUB, _pL, _pL, _V]),
    "rsm_stage_mesh_subdivide_edges": (_I, [_V, _V, _L, _V, _L, _SUB, _V, _V, _V, _V, _pL, _V, _V, _pD]),
    "rsm_mesh_color": (_I, [_V, _V, _L, _V, _L, _VIEW, _I, _COL, _V, _V, _V]),
    "rsm_mesh_color_device": (_I, [_V, _V, _L, _V, _L, _VIEW, _I, _COL, _V, _V, _V]),
    "rsm_mesh_color_last": (_I, [_V, _VIEW, _I, _COL, _V]),
    "rsm_mesh_last_colors": (_I, [_V, _V, _V]),
    "rsm_texture_color": (_I, [_V, _V, _L, _V, _V, _I, _I, _V]),
    "rsm_stage_mesh_depth": (_I, [_V, _V, _L, _V, _L, _V, _I, _I, _V]),
    "rsm_write_ply_mesh_color": (_I, [_S, _V, _L, _V, _L, _V]),
    "rsm_mesh_stitch": (_I, [_V, _V, _L, _V, _L, _VIEW, _I, _COL, _STI, _V, _V, _V]),
    "rsm_mesh_stitch_device": (_I, [_V, _V, _L, _V, _L, _VIEW, _I, _COL, _STI, _V, _V, _V]),
    "rsm_mesh_stitch_last": (_I, [_V, _VIEW, _I, _COL, _STI, _V]),
    "rsm_stage_mesh_visibility": (_I, [_V, _V, _L, _V, _L, _VIEW, _I, _COL, _V]),
    "rsm_stage_mesh_stitch_rhs": (_I, [_V, _V, _L, _V, _L, _VIEW, _I, _V, _V, _V, _I, _V, _V, _V]),
    "rsm_stage_mesh_stitch_solve": (_I, [_V, _V, _L, _L, _V, _V, _V, _D, _I, _V, _pD]),
    "rsm_mesh_fill_colors": (_I, [_V, _V, _L, _L, _V, _V, _V, _FIL, _V]),
    "rsm_mesh_fill_colors_device": (_I, [_V, _V, _L, _L, _V, _V, _V, _FIL, _V]),
    "rsm_mesh_fill_colors_last": (_I, [_V, _FIL, _V]),
    "rsm_stage_mesh_fill_front": (_I, [_V, _V, _L, _L, _V, _V, _I, _I, _V, _V, _pI]),
    "rsm_stage_mesh_fill_solve": (_I, [_V, _V, _L, _L, _V, _I, _I, _V]),
    "rsm_bench_ncc": (_I, [_V, _I, _I, _I, _I, _I, _V]),
}
EXPORTS = list(PROTOTYPES)   # every symbol include/rsm.h declares

_lib = None


def load():
    """Load the HIP library and give every function its prototype; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RsmError(RSM_E_STATE, "librsm_mi355.so not built: run `python -c 'import __graft_entry__ as g; "
                                    "g.build()'` (hipcc, gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    abi = lib.rsm_abi_version()
    if abi != RSM_ABI_VERSION:
        raise RsmError(RSM_E_STATE, "librsm_mi355.so has ABI %d, this binding ABI %d: rebuild the library" % (abi, RSM_ABI_VERSION))
    _lib = lib
    return lib
