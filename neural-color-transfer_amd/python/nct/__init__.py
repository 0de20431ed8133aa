"""nct — thin ctypes binding over libnct.so (the C ABI declared in include/nct.h).

This is plumbing for tests / bench.py only; the product is the shared library + the C++ CLI. There is no CPU
fallback anywhere in this package: if the library is missing or no HIP device is usable, calls raise NctError.
Function names and argument meaning mirror include/nct.h, which cites the reference seam each one replaces
(code/windows/neural_color_transfer/source/main.cu).
"""
import collections
import contextlib
import ctypes as C
import functools
import math
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.normpath(os.path.join(_HERE, "..", ".."))
REPO_ROOT = os.path.normpath(os.path.join(PKG_ROOT, ".."))
LIB_PATH = os.environ.get("NCT_LIB") or os.path.join(PKG_ROOT, "lib", "libnct.so")      # NCT_LIB: kernel-tuning experiments only


class NctError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nct error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libnct.so (in-tree build only — never a site-packages copy)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NctError(-4, f"{LIB_PATH} not found — run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
        if _lib.nct_version() != NCT_VERSION:        # the structs below mirror include/nct.h at this version
            v = _lib.nct_version(); _lib = None
            raise NctError(-2, f"{LIB_PATH} is nct version {v}, this binding was written against {NCT_VERSION}: rebuild")
    return _lib


NCT_VERSION = 118        # include/nct.h
FINISH_EXACT, FINISH_UPSAMPLE = 0, 1      # NCT_FINISH_*: how a full-resolution run reaches the original size (SPEC §6.1 / §6.8)
MAX_REFS = 8             # NCT_MAX_REFS
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")

# name -> (restype, argtypes); the single source of truth for the symbol-export test
SIGNATURES = {
    "nct_version": (C.c_int, []),
    "nct_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "nct_destroy": (None, [C.c_void_p]),
    "nct_last_error": (C.c_char_p, [C.c_void_p]),
    "nct_device_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "nct_ctx_counter": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64)]),
    "nct_synchronize": (C.c_int, [C.c_void_p]),
    "nct_feat_normalize": (C.c_int, [C.c_void_p, _f32p, _f32p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "nct_nnf_init": (C.c_int, [C.c_void_p, _u32p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "nct_nnf_upsample": (C.c_int, [C.c_void_p, _u32p, _u32p] + [C.c_int] * 6),
    "nct_patchmatch": (C.c_int, [C.c_void_p, _f32p, _f32p] + [C.c_int] * 8 + [C.c_uint32, _u32p, _f32p]),
    "nct_bds_vote_features": (C.c_int, [C.c_void_p, _u32p, _u32p, _f32p, _f32p, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_float]),
    "nct_feature_distance": (C.c_int, [C.c_void_p, _f32p, _f32p, _f32p, C.c_int, C.c_int, C.c_int]),
    "nct_bds_vote_image": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _u32p, _u32p, C.c_int, C.c_double, C.c_double, _u8p]),
    "nct_vgg19_load_caffemodel": (C.c_int, [C.c_void_p, C.c_char_p]),
    "nct_model_parse_caffemodel": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "nct_model_free": (None, [C.c_void_p]),
    "nct_model_layer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nct_model_last_error": (C.c_char_p, []),
    "nct_vgg19_load_model": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nct_vgg19_share_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nct_vgg19_weights_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "nct_vgg19_check_prototxt": (C.c_int, [C.c_void_p, C.c_char_p]),
    "nct_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "nct_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "nct_vgg19_load_raw": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int]),
    "nct_vgg19_features": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "nct_conv3x3_relu": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _f32p, C.c_int]),
    "nct_maxpool2x2": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "nct_params_default": (None, [C.c_void_p]),
    "nct_bgr2lab_u8": (C.c_int, [C.c_void_p, _u8p, C.c_size_t, _u8p]),
    "nct_lab2bgr_u8": (C.c_int, [C.c_void_p, _u8p, C.c_size_t, _u8p]),
    "nct_lab2bgr_u8_form": (C.c_int, [C.c_void_p, _u8p, C.c_size_t, _u8p, C.c_int]),
    "nct_resize_u8c3": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int]),
    "nct_resize_f64c3": (C.c_int, [C.c_void_p, _f64p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int]),
    "nct_cluster_features": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, _i32p, C.POINTER(C.c_int)]),
    "nct_knn_graph": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _f64p]),
    "nct_local_color_transfer": (C.c_int, [C.c_void_p, _f32p, _u8p, _u8p, _u8p, _i32p, _f64p] + [C.c_int] * 5 + [C.c_void_p, _u8p, C.c_void_p]),
    "nct_process_pair": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p]),
    "nct_working_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nct_process_pair_fullres": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p]),
    "nct_color_finish": (C.c_int, [C.c_void_p, _f64p] + [C.c_int] * 4 + [_u8p, C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p]),
    "nct_process_pair_fullres_finish": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _u8p, C.c_void_p]),
    "nct_guided_params_default": (None, [C.c_void_p]),
    "nct_set_finish_guided": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nct_pair_upload": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int]),
    "nct_pair_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_pair_run_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_pair_download": (C.c_int, [C.c_void_p, _u8p]),
    "nct_multi_upload": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nct_multi_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_multi_run_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_multi": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, _u8p, C.c_void_p]),
    "nct_seq_params_default": (None, [C.c_void_p]),
    "nct_seq_begin": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nct_seq_begin_fullres": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nct_seq_hold_default": (None, [C.c_void_p]),
    "nct_seq_begin_multi": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_begin_multi_fullres": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "nct_seq_frame_multi_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_multi_stage_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p]),
    "nct_seq_frame_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_propagate": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p]),
    "nct_seq_frame_propagate_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p]),
    "nct_seq_reset": (C.c_int, [C.c_void_p]),
    "nct_seq_end": (C.c_int, [C.c_void_p]),
    "nct_seq_motion_default": (None, [C.c_void_p]),
    "nct_seq_set_motion": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nct_seq_set_carry": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "nct_seq_get_carry": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nct_seq_auto_default": (None, [C.c_void_p]),
    "nct_seq_probe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_auto": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_lut_params_default": (None, [C.c_void_p]),
    "nct_pair_fit_lut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_lut_accum_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "nct_lut_accum_add_run": (C.c_int, [C.c_void_p]),
    "nct_lut_accum_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_lut_accum_end": (C.c_int, [C.c_void_p]),
    "nct_grid_params_default": (None, [C.c_void_p]),
    "nct_pair_fit_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_region_params_default": (None, [C.c_void_p]),
    "nct_pair_set_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_pair_run_region_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_pair_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_pair_fullres_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_pair_fullres_finish_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_void_p]),
    "nct_seq_set_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_set_ref_region": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_ref_region_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_propagate_ref_region_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_region_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_set_region_tracking": (C.c_int, [C.c_void_p, C.c_int]),
    "nct_seq_get_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_region_snap_params_default": (None, [C.c_void_p]),
    "nct_seq_set_region_snap": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nct_region_select_params_default": (None, [C.c_void_p]),
    "nct_region_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_region_select_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_region_score_bench": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_float)]),
    "nct_pair_select_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_select_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_region_refind_params_default": (None, [C.c_void_p]),
    "nct_region_model_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nct_region_model_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nct_region_model_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nct_region_model_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "nct_region_model_from_rows": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "nct_region_model_free": (None, [C.c_void_p]),
    "nct_reflib_params_default": (None, [C.c_void_p]),
    "nct_reflib_create": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nct_reflib_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "nct_reflib_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "nct_reflib_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "nct_reflib_from_rows": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "nct_reflib_free": (None, [C.c_void_p]),
    "nct_reflib_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_reflib_release": (C.c_int, [C.c_void_p]),
    "nct_descriptor_match_bench": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "nct_region_refind_bench": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "nct_region_model_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_region_model_apply_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_pair_apply_region_model": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_set_region_model": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_seq_frame_propagate_region_levels": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_pair_set_ref_region": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nct_multi_run_ref_region_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_pair_run_ref_region_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_pair_ref_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_multi_ref_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p),
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nct_process_pair_fullres_ref_region": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]),
    "nct_dev_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "nct_dev_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "nct_dev_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "nct_dev_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "nct_chw_to_hwc_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "nct_hwc_to_chw_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "nct_vgg19_features_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]),
    "nct_vgg19_features_hwc_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "nct_feat_normalize_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "nct_nnf_init_dev": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 4),
    "nct_nnf_upsample_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6),
    "nct_patchmatch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_uint32, C.c_void_p, C.c_void_p]),
    "nct_patchmatch_bidir_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "nct_bds_vote_features_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_float]),
    "nct_bds_vote_image_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_double, C.c_double, C.c_void_p]),
    "nct_feature_distance_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "nct_conv3x3_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "nct_conv3x3_pair_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "nct_pm_bench_setup": (C.c_int, [C.c_void_p, _f32p, _f32p] + [C.c_int] * 5),
    "nct_pm_bench_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]),
    "nct_pm_bench_run_bidir": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


class _voidp(C.c_void_p):
    """void* as an argument type: an address, None, or the array that stands there (no dtype is checked: the host and the device form of a seam share their row)"""

    @classmethod
    def from_param(cls, v):
        return C.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else C.c_void_p.from_param(v)


_P, _I, _D, _N, _L = _voidp, C.c_int, C.c_double, C.c_size_t, C.POINTER(C.c_void_p)
# the seams whose nct_X and nct_X_dev take the same list, pointers to host memory in one and to arena blocks in the other: one row, both names (nct_region_select and
# nct_region_model_apply, whose host forms take a stages struct more, keep two rows above)
_TWINS = {
    "nct_color_finish_upsample": [_P, _I, _I, _P, _I, _I, _P, _P],
    "nct_color_finish_guided": [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P],
    "nct_color_finish_upsample_region": [_P, _I, _I, _P, _I, _I, _P, _P, _P, _P],
    "nct_color_finish_guided_region": [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P],
    "nct_select_reference": [_L, _L, _I, _I, _I, _P, _P, _P],
    "nct_select_reference_hold": [_L, _L, _I, _I, _I, _P, _P, _P, _P, _D, _D, _P, _P, _P, _P, _P],
    "nct_region_pull": [_P, _I, _I, _P, _P, _I, _I, _D, _D, _P],
    "nct_seq_warp": [_P, _I, _I, _P, _P],
    "nct_seq_blend": [_P, _P, _P, _P, _I, _I, _D, _D, _P, _P],
    "nct_seq_blend_mc": [_P, _P, _P, _P, _I, _I, _D, _D, _P, _P, _P],
    "nct_seq_motion_field": [_P, _P, _I, _I, _P, _I, _I, _I, _I, _P],
    "nct_seq_change": [_P, _P, _I, _I, _P, _I, _P],
    "nct_seq_pull_hold": [_L, _I, _P, _P, _P, _P, _P, _P, _I, _I, _D, _D, _P, _P, _P],
    "nct_seq_matte_warp": [_P, _I, _I, _P, _I, _I, _P],
    "nct_lut_fit": [_P, _P, _N, _P, _P, _P],
    "nct_lut_fit_masked": [_P, _P, _P, _N, _P, _P, _P],
    "nct_lut_apply": [_P, _I, _P, _N, _P],
    "nct_lut_apply_u16": [_P, _I, _P, _N, _P],
    "nct_lut_accum_add": [_P, _P, _P, _N],
    "nct_lut_accum_solve": [_D, _P, _P],
    "nct_grid_fit": [_P, _P, _I, _I, _P, _P, _P],
    "nct_grid_apply": [_P, _I, _I, _I, _P, _I, _I, _P],
    "nct_grid_apply_u16": [_P, _I, _I, _I, _P, _I, _I, _P],
    "nct_resize_u8c1": [_P, _I, _I, _P, _I, _I],
    "nct_region_mix": [_P, _P, _I, _I, _P],
    "nct_region_compose": [_P, _P, _P, _N, _P, _P, _P],
    "nct_region_snap": [_P, _P, _I, _I, _P, _P],
    "nct_feat_quantize": [_P, _P, _I, _I, _I],
    "nct_region_score": [_P, _I, _I, _P, _I, _P, _I, _I, _I, _P],
    "nct_region_refind": [_P, _I, _I, _P, _I, _I, _I, _P],
    "nct_feat_quantize8": [_P, _P, _P, _I, _I, _I],
    "nct_descriptor_match": [_P, _I, _I, _P, _P, _I, _P, _P],              # offsets: a host array in both forms
    "nct_nnf_carry": [_P, _I, _I, _P, _P],
    "nct_nnf_forward_map": [_P, _I, _I, _P],
    "nct_nnf_remap": [_P, _I, _I, _P, _I, _I, _P],
    "nct_nnf_merge": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P],
}
for _name, _args in _TWINS.items():
    SIGNATURES[_name] = SIGNATURES[_name + "_dev"] = (C.c_int, [C.c_void_p] + _args)


def _declare(l):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype = res
        fn.argtypes = args


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Params(C.Structure):
    """struct nct_params (include/nct.h)."""
    _fields_ = [("bds_weight", C.c_double), ("eps", C.c_double), ("nonlocal_weight", C.c_double), ("local_weight", C.c_double),
                ("wls_lambda_init", C.c_double), ("cluster_num", C.c_int), ("k_num", C.c_int), ("patch_size", C.c_int),
                ("wls_alpha", C.c_double), ("pm_iters", C.c_int), ("seed", C.c_uint32), ("levels", C.c_int), ("flags", C.c_uint32)]

    @staticmethod
    def default():
        p = Params()
        lib().nct_params_default(C.byref(p))
        return p


class PairTiming(C.Structure):
    """struct nct_pair_timing (include/nct.h)."""
    _fields_ = [("total_ms", C.c_double), ("vgg_ms", C.c_double), ("cluster_ms", C.c_double), ("patchmatch_ms", C.c_double),
                ("vote_ms", C.c_double), ("knn_ms", C.c_double), ("color_ms", C.c_double), ("other_ms", C.c_double),
                ("nonlocal_ms", C.c_double), ("wls_ms", C.c_double), ("wls_iters", C.c_int * 5),
                ("pm_level_ms", C.c_double * 5), ("pm_level_launches", C.c_int * 5),
                ("vote_level_ms", C.c_double * 5), ("nonlocal_level_ms", C.c_double * 5), ("wls_level_ms", C.c_double * 5),
                ("pm_level_evals", C.c_ulonglong * 5), ("pm_level_accepted", C.c_ulonglong * 5),
                ("kernel_us", C.c_double * 10), ("kernel_samples", C.c_int * 10)]

    def as_dict(self):
        d = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            d[k] = v if isinstance(v, (int, float)) else list(v)
        return d


CTR_ARENA_BYTES, CTR_S1_HUB_BLOCKS_L0 = 0, 1
FLAG_FEAT16 = 1
FLAG_COUNT_EVALS = 2
FLAG_LATENCY = 4
FLAG_LAB2BGR_CUBE = 8
FLAG_TIME_KERNELS = 16
KT_NAMES = ("s1_apply", "s1_scalars", "s1_update", "wls_down", "wls_up", "wls_apply", "wls_update", "wls_coarse", "wls_block_pre", "wls_block_post")      # nct.h NCT_KT_*
LAB2BGR_PIECEWISE, LAB2BGR_CUBE = 0, 1


def working_size(h, w, max_side=1000):
    """nct_working_size (SPEC §6.1 rule 1 + the limits of rule 5; no GPU needed): the (h, w) the pyramid runs at; NctError when refused"""
    wh, ww = C.c_int(), C.c_int()
    rc = lib().nct_working_size(h, w, max_side, C.byref(wh), C.byref(ww))
    if rc != 0:
        raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
    return wh.value, ww.value


class Model:
    """host-side parsed caffemodel (nct_model): parse the file once per process, upload it once per GPU (Context.vgg19_load_model)."""

    def __init__(self, path):
        self._m = None
        m = C.c_void_p()
        rc = lib().nct_model_parse_caffemodel(os.fsencode(path), C.byref(m))
        if rc != 0:
            raise NctError(rc, (lib().nct_model_last_error() or b"").decode())
        self._m = m

    def layer(self, i):
        """(weights [cout, cin, 3, 3], bias [cout]) of conv layer i (0 = conv1_1 … 12 = conv5_1) as numpy copies (nct_model_layer)"""
        w, b, co, ci = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int(), C.c_int()
        rc = lib().nct_model_layer(self._m, i, C.byref(w), C.byref(b), C.byref(co), C.byref(ci))
        if rc != 0:
            raise NctError(rc, (lib().nct_model_last_error() or b"").decode())
        return (np.ctypeslib.as_array(w, (co.value, ci.value, 3, 3)).copy(), np.ctypeslib.as_array(b, (co.value,)).copy())

    def close(self):
        if self._m:
            lib().nct_model_free(self._m); self._m = None

    def __del__(self):
        self.close()


def check_prototxt(path):
    """nct_vgg19_check_prototxt without a context (no GPU needed): raises NctError with the reason when the file is not this library's VGG19"""
    rc = lib().nct_vgg19_check_prototxt(None, os.fsencode(path))
    if rc != 0:
        raise NctError(rc, (lib().nct_model_last_error() or b"").decode())


class PairLevels(C.Structure):
    """struct nct_pair_levels (include/nct.h)."""
    _fields_ = [(k, C.c_void_p * 5) for k in ("ann", "bnn", "annd", "bnnd", "guide", "err", "result", "color")] + [("labels", C.c_void_p)]


class MultiLevels(C.Structure):
    """struct nct_multi_levels (include/nct.h)."""
    _fields_ = [(k, (C.c_void_p * 5) * MAX_REFS) for k in ("ann", "bnn", "annd", "bnnd", "ref_guide", "ref_err")] + \
               [(k, C.c_void_p * 5) for k in ("label", "guide", "err", "result")] + [("labels", C.c_void_p)]


class LutParams(C.Structure):
    """struct nct_lut_params (include/nct.h)."""
    _fields_ = [("size", C.c_int), ("lambda_", C.c_double)]

    @staticmethod
    def default():
        p = LutParams()
        lib().nct_lut_params_default(C.byref(p))
        return p


class LutStages(C.Structure):
    """struct nct_lut_stages (include/nct.h)."""
    _fields_ = [("weight", C.c_void_p), ("resid", C.c_void_p), ("disp", C.c_void_p)]


def _lut_params(size, lam):
    p = LutParams.default()
    if size is not None:
        p.size = int(size)
    if lam is not None:
        p.lambda_ = float(lam)
    return p


class GridParams(C.Structure):
    """struct nct_grid_params (include/nct.h)."""
    _fields_ = [("gy", C.c_int), ("gx", C.c_int), ("gz", C.c_int), ("lambda_", C.c_double)]

    @staticmethod
    def default():
        p = GridParams()
        lib().nct_grid_params_default(C.byref(p))
        return p


class GridStages(C.Structure):
    """struct nct_grid_stages (include/nct.h)."""
    _fields_ = [("sums", C.c_void_p), ("blurred", C.c_void_p)]


def _grid_params(shape, lam):
    p = GridParams.default()
    if shape is not None:
        p.gy, p.gx, p.gz = (int(v) for v in shape)
    if lam is not None:
        p.lambda_ = float(lam)
    return p


def _grid_host_shape(gy, gx, gz):
    """the shape of the host arrays of a grid: a refused node count never reaches them, so it only has to exist"""
    return (gy, gx, gz) if 0 < gy <= 64 and 0 < gx <= 64 and 0 < gz <= 32 else (1, 1, 1)


class GuidedParams(C.Structure):
    """struct nct_guided_params (include/nct.h)."""
    _fields_ = [("sigma", C.c_double)]

    @staticmethod
    def default():
        p = GuidedParams()
        lib().nct_guided_params_default(C.byref(p))
        return p


def _guided_params(sigma):
    p = GuidedParams.default()
    if sigma is not None:
        p.sigma = float(sigma)
    return p


class RegionParams(C.Structure):
    """struct nct_region_params (include/nct.h)."""
    _fields_ = [("protect", C.c_int)]

    @staticmethod
    def default():
        p = RegionParams()
        lib().nct_region_params_default(C.byref(p))
        return p


class RegionLevels(C.Structure):
    """struct nct_region_levels (include/nct.h)."""
    _fields_ = [("ab_mix", C.c_void_p * 5), ("mask", C.c_void_p * 5)]


class RefRegionLevels(C.Structure):
    """struct nct_ref_region_levels (include/nct.h)."""
    _fields_ = [("ref_mask", (C.c_void_p * 5) * MAX_REFS), ("pulled", (C.c_void_p * 5) * MAX_REFS), ("mask", C.c_void_p * 5), ("mask_full", C.c_void_p * 5), ("ab_mix", C.c_void_p * 5)]


def _region_params(protect):
    p = RegionParams.default()
    if protect is not None:
        p.protect = int(protect)
    return p


class RegionSnapParams(C.Structure):
    """struct nct_region_snap_params (include/nct.h)."""
    _fields_ = [("radius", C.c_int), ("sigma", C.c_int), ("binary", C.c_int)]

    @staticmethod
    def default():
        p = RegionSnapParams()
        lib().nct_region_snap_params_default(C.byref(p))
        return p


def _snap_params(radius, sigma, binary):
    p = RegionSnapParams.default()
    if radius is not None:
        p.radius = int(radius)
    if sigma is not None:
        p.sigma = int(sigma)
    if binary is not None:
        p.binary = int(binary)
    return p


STROKE_IN, STROKE_OUT = 255, 128                          # nct.h NCT_STROKE_*


class RegionSelectParams(C.Structure):
    """struct nct_region_select_params (include/nct.h)."""
    _fields_ = [("tap", C.c_int), ("sharpness", C.c_int), ("floor_permille", C.c_int), ("max_seeds", C.c_int), ("snap_iters", C.c_int), ("snap", RegionSnapParams)]

    @staticmethod
    def default():
        p = RegionSelectParams()
        lib().nct_region_select_params_default(C.byref(p))
        return p


class RegionSelectStages(C.Structure):
    """struct nct_region_select_stages (include/nct.h)."""
    _fields_ = [("q", C.c_void_p), ("cell", C.c_void_p), ("score", C.c_void_p), ("up", C.c_void_p)]


def region_select_params(tap=None, sharpness=None, floor_permille=None, max_seeds=None, snap_iters=None, radius=None, sigma=None, binary=None):
    """struct nct_region_select_params with nct_region_select_params_default's values (2, 1024, 700, 4096, 1, snap 3 / 10 / 1) where an argument is left out"""
    p = RegionSelectParams.default()
    for k, v in (("tap", tap), ("sharpness", sharpness), ("floor_permille", floor_permille), ("max_seeds", max_seeds), ("snap_iters", snap_iters)):
        if v is not None:
            setattr(p, k, int(v))
    for k, v in (("radius", radius), ("sigma", sigma), ("binary", binary)):
        if v is not None:
            setattr(p.snap, k, int(v))
    return p


class RegionRefindParams(C.Structure):
    """struct nct_region_refind_params (include/nct.h)."""
    _fields_ = [("sharpness", C.c_int), ("floor_permille", C.c_int), ("margin", C.c_int), ("snap_iters", C.c_int), ("snap", RegionSnapParams)]

    @staticmethod
    def default():
        p = RegionRefindParams()
        lib().nct_region_refind_params_default(C.byref(p))
        return p


class RegionApplyStages(C.Structure):
    """struct nct_region_apply_stages (include/nct.h)."""
    _fields_ = [("q", C.c_void_p), ("score", C.c_void_p), ("refound", C.c_void_p)]


def region_refind_params(sharpness=None, floor_permille=None, margin=None, snap_iters=None, radius=None, sigma=None, binary=None):
    """struct nct_region_refind_params with nct_region_refind_params_default's values (1024, 700, 32, 1, snap 3 / 10 / 1) where an argument is left out"""
    p = RegionRefindParams.default()
    for k, v in (("sharpness", sharpness), ("floor_permille", floor_permille), ("margin", margin), ("snap_iters", snap_iters)):
        if v is not None:
            setattr(p, k, int(v))
    for k, v in (("radius", radius), ("sigma", sigma), ("binary", binary)):
        if v is not None:
            setattr(p.snap, k, int(v))
    return p


class RegionModel:
    """nct_region_model (SPEC §6.17): the kept seed rows of a selection from strokes, a host object without a context. Made by Context.region_model_fit or from rows
    the caller holds (rows_in [n_in, C], rows_out [n_out, C] or None, int16: nct_region_model_from_rows)."""

    def __init__(self, tap=None, rows_in=None, rows_out=None, _handle=None):
        self._m = None
        if _handle is not None:
            self._m = _handle
            return
        ri = np.ascontiguousarray(rows_in, np.int16)
        ro = None if rows_out is None or len(rows_out) == 0 else np.ascontiguousarray(rows_out, np.int16)
        if ri.ndim != 2 or (ro is not None and (ro.ndim != 2 or ro.shape[1] != ri.shape[1])):
            raise NctError(-2, "RegionModel: rows_in must be [n_in, C] int16 and rows_out [n_out, C] or None")
        m = C.c_void_p()
        rc = lib().nct_region_model_from_rows(int(tap), ri.shape[1], ri.ctypes.data, ri.shape[0], None if ro is None else ro.ctypes.data, 0 if ro is None else ro.shape[0], C.byref(m))
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        self._m = m

    def info(self):
        """nct_region_model_info -> (tap, C, n_in, n_out)"""
        v = [C.c_int() for _ in range(4)]
        rc = lib().nct_region_model_info(self._m, *[C.byref(x) for x in v])
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        return tuple(x.value for x in v)

    def rows(self):
        """nct_region_model_rows -> (rows_in [n_in, C], rows_out [n_out, C]) as numpy copies"""
        _, Cc, n_in, n_out = self.info()
        a, b = C.c_void_p(), C.c_void_p()
        rc = lib().nct_region_model_rows(self._m, C.byref(a), C.byref(b))
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        def arr(ptr, n):
            if n == 0:
                return np.zeros((0, Cc), np.int16)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int16)), (n, Cc)).copy()
        return arr(a, n_in), arr(b, n_out)

    def close(self):
        if self._m:
            lib().nct_region_model_free(self._m); self._m = None

    def __del__(self):
        self.close()


class RefLibParams(C.Structure):
    """struct nct_reflib_params (include/nct.h)."""
    _fields_ = [("wf", C.c_int), ("wb", C.c_int)]

    @staticmethod
    def default():
        p = RefLibParams()
        lib().nct_reflib_params_default(C.byref(p))
        return p


class RefLib:
    """nct_reflib (SPEC §6.21): the int8 tap descriptors of a library's entries, a host object without a context. RefLib(tap, center=None) is empty
    (nct_reflib_create; C is the tap's channel count); RefLib.from_rows(tap, rows, offsets, center=None) holds rows the caller has (nct_reflib_from_rows)."""

    TAP_C = (64, 128, 256, 512, 512)

    def __init__(self, tap, center=None, C_=None, _handle=None):
        self._m = None
        if _handle is not None:
            self._m = _handle
            return
        mu = None if center is None else np.ascontiguousarray(center, np.float32)
        Cc = int(C_) if C_ is not None else (self.TAP_C[tap - 1] if 1 <= tap <= 5 else 0)
        if mu is not None and mu.shape != (Cc,):
            raise NctError(-2, "RefLib: center must be [C] fp32")
        m = C.c_void_p()
        rc = lib().nct_reflib_create(int(tap), Cc, None if mu is None else mu.ctypes.data, C.byref(m))
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        self._m = m

    @classmethod
    def from_rows(cls, tap, rows, offsets, center=None):
        r, o = np.ascontiguousarray(rows, np.int8), np.ascontiguousarray(offsets, np.int32)
        mu = None if center is None else np.ascontiguousarray(center, np.float32)
        if r.ndim != 2 or o.ndim != 1 or o.size < 1 or (mu is not None and mu.shape != (r.shape[1],)):
            raise NctError(-2, "RefLib.from_rows: rows must be [total, C] int8, offsets [N + 1] int32 and center [C] fp32 or None")
        m = C.c_void_p()
        rc = lib().nct_reflib_from_rows(int(tap), r.shape[1], None if mu is None else mu.ctypes.data, r.ctypes.data, o.ctypes.data, o.size - 1, C.byref(m))
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        return cls(tap, _handle=m)

    def info(self):
        """nct_reflib_info -> (tap, C, N, total rows, centred)"""
        tap, Cc, N, tot, cen = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        rc = lib().nct_reflib_info(self._m, C.byref(tap), C.byref(Cc), C.byref(N), C.byref(tot), C.byref(cen))
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        return tap.value, Cc.value, N.value, tot.value, bool(cen.value)

    def rows(self):
        """nct_reflib_rows -> (rows [total, C] int8, offsets [N + 1] int32, center [C] fp32 or None) as numpy copies"""
        _, Cc, N, tot, cen = self.info()
        r, o, mu = C.c_void_p(), C.c_void_p(), C.c_void_p()
        rc = lib().nct_reflib_rows(self._m, C.byref(r), C.byref(o), C.byref(mu))
        if rc != 0:
            raise NctError(rc, (lib().nct_last_error(None) or b"").decode())
        rows = np.ctypeslib.as_array(C.cast(r, C.POINTER(C.c_int8)), (tot, Cc)).copy() if tot else np.zeros((0, Cc), np.int8)
        offs = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_int32)), (N + 1,)).copy()
        return rows, offs, (np.ctypeslib.as_array(C.cast(mu, C.POINTER(C.c_float)), (Cc,)).copy() if cen else None)

    def add(self, ctx, bgr):
        """nct_reflib_add: bgr [h, w, 3] becomes the next entry (one forward to the tap on ctx, rule D2)"""
        img = np.ascontiguousarray(bgr, np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise NctError(-2, "RefLib.add: bgr must be [h, w, 3] bytes")
        ctx._chk(ctx._l.nct_reflib_add(ctx._h, self._m, img.ctypes.data, img.shape[0], img.shape[1]))

    def close(self):
        if self._m:
            lib().nct_reflib_free(self._m); self._m = None

    def __del__(self):
        self.close()


def _mask_arg(mask, shape, what):
    """a region mask as contiguous bytes of its image's h x w (shape: that image's); a mask of another size is refused here: the C entry points take the image's size for it"""
    m = np.ascontiguousarray(mask, np.uint8)
    if m.shape != tuple(shape[:2]):
        raise NctError(-2, f"{what}: mask is {m.shape[1] if m.ndim == 2 else '?'}x{m.shape[0] if m.ndim else '?'}, its image {shape[1]}x{shape[0]}")
    return m


class SeqParams(C.Structure):
    """struct nct_seq_params (include/nct.h)."""
    _fields_ = [("tau", C.c_double), ("sigma", C.c_double)]

    @staticmethod
    def default():
        p = SeqParams()
        lib().nct_seq_params_default(C.byref(p))
        return p


class SeqHold(C.Structure):
    """struct nct_seq_hold (include/nct.h; SPEC §6.18)."""
    _fields_ = [("hold", C.c_double)]

    @staticmethod
    def default():
        p = SeqHold()
        lib().nct_seq_hold_default(C.byref(p))
        return p


class SeqHoldLevels(C.Structure):
    """struct nct_seq_hold_levels (include/nct.h)."""
    _fields_ = [("free_label", C.c_void_p * 5), ("margin", C.c_void_p * 5)]


class SeqPullLevels(C.Structure):
    """struct nct_seq_pull_levels (include/nct.h; SPEC §6.19)."""
    _fields_ = [("p_free", C.c_void_p * 5), ("p_held", C.c_void_p * 5)]


class SeqLevels(C.Structure):
    """struct nct_seq_levels (include/nct.h)."""
    _fields_ = [("ab_blend", C.c_void_p * 5), ("tau_map", C.c_void_p * 5), ("motion", C.c_void_p * 5)]


class SeqMotion(C.Structure):
    """struct nct_seq_motion (include/nct.h)."""
    _fields_ = [("radius0", C.c_int), ("radius", C.c_int), ("penalty", C.c_int)]

    @staticmethod
    def default():
        p = SeqMotion()
        lib().nct_seq_motion_default(C.byref(p))
        return p


class SeqChange(C.Structure):
    """struct nct_seq_change_rec (include/nct.h)."""
    _fields_ = [("sad", C.c_uint64), ("changed", C.c_uint32), ("pixels", C.c_uint32)]

    def as_dict(self):
        return {"sad": int(self.sad), "changed": int(self.changed), "pixels": int(self.pixels)}


class SeqAuto(C.Structure):
    """struct nct_seq_auto (include/nct.h)."""
    _fields_ = [("threshold", C.c_int), ("cut_permille", C.c_int), ("key_permille", C.c_int), ("max_gap", C.c_int)]

    @staticmethod
    def default():
        p = SeqAuto()
        lib().nct_seq_auto_default(C.byref(p))
        return p


SEQ_FIRST, SEQ_PROPAGATED, SEQ_KEY, SEQ_CUT = 0, 1, 2, 3        # nct.h NCT_SEQ_*


class SeqDecision(C.Structure):
    """struct nct_seq_decision (include/nct.h)."""
    _fields_ = [("kind", C.c_int), ("level", C.c_int), ("change", SeqChange), ("acc_changed", C.c_uint32), ("gap", C.c_int), ("probe_ms", C.c_double)]

    def as_dict(self):
        d = {"kind": self.kind, "level": self.level, "acc_changed": int(self.acc_changed), "gap": self.gap, "probe_ms": self.probe_ms}
        d.update(self.change.as_dict())
        return d


def seq_auto(threshold=None, cut_permille=None, key_permille=None, max_gap=None):
    """struct nct_seq_auto with nct_seq_auto_default's values (24, 500, 100, 8) where an argument is left out"""
    p = SeqAuto.default()
    for k, v in (("threshold", threshold), ("cut_permille", cut_permille), ("key_permille", key_permille), ("max_gap", max_gap)):
        if v is not None:
            setattr(p, k, int(v))
    return p


class ColorStages(C.Structure):
    """struct nct_color_stages (include/nct.h)."""
    _fields_ = [("ab_local", C.c_void_p), ("ab_nonlocal", C.c_void_p), ("ab_up", C.c_void_p), ("roughness", C.c_void_p),
                ("ab_wls", C.c_void_p), ("cg_iters", C.c_void_p), ("wls_iters", C.c_void_p)]


# ---- the level reports: the host arrays the report structs above point into, described once per field and allocated by one function
def _level_dims(h, w):
    """the five level grids (h, w) of an h x w image, coarsest first"""
    dims = []
    for _ in range(5):
        dims.insert(0, (h, w)); h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return dims


# src[l] / ref[k][l]: the level grids of the source and of reference k; work: the size the pyramid runs at; finish[l]: the size level l's finish targets
_Grids = collections.namedtuple("_Grids", "src ref work finish")


def _grids(src_shape, ref_shapes, finish=None):
    H, W = src_shape[:2]
    return _Grids(_level_dims(H, W), [_level_dims(*r[:2]) for r in ref_shapes], (H, W), finish or [(H, W)] * 5)


_SHAPES = {                                                       # the grid a field lives on -> its shape at level l (of reference k)
    "src": lambda g, l, k: g.src[l],                              # a map on the source level
    "src3": lambda g, l, k: g.src[l] + (3,),                      # an image on the source level
    "ref": lambda g, l, k: g.ref[k][l],                           # a map on the reference level
    "coef": lambda g, l, k: (2, g.src[l][0] * g.src[l][1], 3),    # a coefficient map [2, h*w, 3] of the source level
    "field": lambda g, l, k: g.src[l] + (2,),                     # a field of (my, mx) on the source level
    "work3": lambda g, l, k: g.work + (3,),                       # an image at the working size
    "work_coef": lambda g, l, k: (2, g.work[0] * g.work[1], 3),   # a coefficient map of the working size
    "work_flat": lambda g, l, k: (g.work[0] * g.work[1],),        # a value per working-size pixel
    "finish": lambda g, l, k: g.finish[l],                        # a map at the size the level's finish targets
}
ALL, RUN, ONE = "all five levels", "the levels that run", "one array"
# a report field: its dtype; its grid (a _SHAPES key, or a fixed shape); whether the struct holds it per reference ([k][l]); the levels it spans
_Field = collections.namedtuple("_Field", "dtype grid per_ref span", defaults=(False, ALL))
_REPORT = {                                                       # struct -> field -> _Field, in the struct's order. PairLevels.color points at ColorStages: _pair_report
    PairLevels: {"ann": _Field(np.uint32, "src"), "bnn": _Field(np.uint32, "ref"), "annd": _Field(np.float32, "src"), "bnnd": _Field(np.float32, "ref"),
                 "guide": _Field(np.uint8, "src3"), "err": _Field(np.float32, "src"), "result": _Field(np.uint8, "work3"), "labels": _Field(np.int32, "src", span=ONE)},
    MultiLevels: {"ann": _Field(np.uint32, "src", True), "bnn": _Field(np.uint32, "ref", True), "annd": _Field(np.float32, "src", True), "bnnd": _Field(np.float32, "ref", True),
                  "ref_guide": _Field(np.uint8, "src3", True), "ref_err": _Field(np.float32, "src", True), "label": _Field(np.uint8, "src"), "guide": _Field(np.uint8, "src3"),
                  "err": _Field(np.float32, "src"), "result": _Field(np.uint8, "work3"), "labels": _Field(np.int32, "src", span=ONE)},
    ColorStages: {"ab_local": _Field(np.float64, "coef", span=ONE), "ab_nonlocal": _Field(np.float64, "coef", span=ONE), "ab_up": _Field(np.float64, "work_coef", span=ONE),
                  "roughness": _Field(np.float64, "work_flat", span=ONE), "ab_wls": _Field(np.float64, "work_coef", span=ONE), "cg_iters": _Field(np.int32, (3,), span=ONE),
                  "wls_iters": _Field(np.int32, (6,), span=ONE)},
    SeqLevels: {"ab_blend": _Field(np.float64, "coef", span=RUN), "tau_map": _Field(np.float64, "src", span=RUN), "motion": _Field(np.int16, "field", span=RUN)},
    SeqHoldLevels: {"free_label": _Field(np.uint8, "src", span=RUN), "margin": _Field(np.float64, "src", span=RUN)},
    RegionLevels: {"ab_mix": _Field(np.float64, "coef", span=RUN), "mask": _Field(np.uint8, "src")},
    RefRegionLevels: {"ref_mask": _Field(np.uint8, "ref", True, RUN), "pulled": _Field(np.uint8, "src", True, RUN), "mask": _Field(np.uint8, "src", span=RUN),
                      "mask_full": _Field(np.uint8, "finish", span=RUN), "ab_mix": _Field(np.float64, "coef", span=RUN)},
    SeqPullLevels: {"p_free": _Field(np.uint8, "src", span=RUN), "p_held": _Field(np.uint8, "src", span=RUN)},
}


def _report(cls, g, levels=5, level=0):
    """the arrays a report struct points into on the grids g -> (dict of them by field, zero-filled; the struct, its pointers set). levels: how many levels run (a RUN
    field stops there); level: the level a ONE field describes"""
    keep, st = {}, cls()
    for name, f in _REPORT[cls].items():
        def new(l, k=0):
            return np.zeros(f.grid if isinstance(f.grid, tuple) else _SHAPES[f.grid](g, l, k), f.dtype)
        n = levels if f.span == RUN else 5
        if f.span == ONE:
            keep[name] = new(level)
            setattr(st, name, keep[name].ctypes.data)
        elif f.per_ref:
            keep[name] = [[new(l, k) for l in range(n)] for k in range(len(g.ref))]
            for k, row in enumerate(keep[name]):
                for l, a in enumerate(row):
                    getattr(st, name)[k][l] = a.ctypes.data
        else:
            keep[name] = [new(l) for l in range(n)]
            for l, a in enumerate(keep[name]):
                getattr(st, name)[l] = a.ctypes.data
    return keep, st


def _reports(g, levels, *classes):
    """several report structs on the same grids -> (one dict of all their arrays, the structs in that order)"""
    keep, structs = {}, []
    for cls in classes:
        more, st = _report(cls, g, levels)
        keep.update(more); structs.append(st)
    return keep, structs


def _multi_reports(g, levels, *more):
    """MultiLevels and the structs in `more` -> _reports' pair, with the grids as "adims" ([l]) and "bdims" ([k][l])"""
    keep, structs = _reports(g, levels, MultiLevels, *more)
    keep["adims"], keep["bdims"] = g.src, g.ref
    return keep, structs


def _color_stages(g, n, levels):
    """the colour stage's report of the n coarsest levels -> (a dict of arrays per level; the void*[5] of nct_color_stages, set for the levels that run; the structs
    it points at, which the caller holds until its call has returned)"""
    made = [_report(ColorStages, g, level=l) for l in range(n)]
    structs = [st for _, st in made]
    return [d for d, _ in made], (C.c_void_p * 5)(*[C.addressof(st) if i < levels else None for i, st in enumerate(structs)]), structs


def _pair_report(g, levels, want_color):
    """PairLevels -> (dict of its arrays + "dims", the struct, what must stay alive until the call returns). want_color: "color" for all five levels, wired for the
    levels that run, and "labels"; without it both pointers stay NULL"""
    keep, lv = _report(PairLevels, g)
    hold = None
    if want_color:
        keep["color"], lv.color, hold = _color_stages(g, 5, levels)
    else:
        del keep["labels"]
        lv.labels = None
    keep["dims"] = [a + b for a, b in zip(g.src, g.ref[0])]
    return keep, lv, hold


# the open sequence as the binding knows it: the (h, w) the frames and each reference arrive at, the (h, w) the pyramid runs at (the same unless the sequence is
# full-resolution), the levels that run, and the finish of a full-resolution sequence (None otherwise)
_Seq = collections.namedtuple("_Seq", "arrive ref_arrive work ref_work levels finish")


class _Blocks:
    """what Context.blocks() hands out: the arena blocks taken through it, in `held`"""

    def __init__(self, ctx):
        self._c, self.held = ctx, []

    def up(self, a):
        self.held.append(self._c.dev_upload(a)); return self.held[-1]

    def new(self, nbytes):
        self.held.append(self._c.dev_alloc(nbytes)); return self.held[-1]

    def free(self, p):
        self.held.remove(p); self._c.dev_free(p)


# an array a seam call has staged: ptr goes into the call (a host address, or an arena block); arr is the host array (None for a block that was only reserved); shape and
# dtype are what get() hands back
_Staged = collections.namedtuple("_Staged", "ptr arr shape dtype")


class _Seam:
    """The binding's counterpart of HostCall (csrc/nct_internal.h): the staging of one call of a seam that exists as nct_X and nct_X_dev, so that the seam's method is
    written once for both forms. Host form (blocks None): an input is kept alive and its address handed over, an output is an np.empty. Device form: an input goes
    through dev_upload, an output is a dev_alloc of its byte size, get() is a dev_download. The arena is asked for blocks in the order of the put() / new() calls. Where
    the two forms differ today, the difference is an argument here (upload, dev_shape, nbytes, fill, over(), host_only), never a second body"""

    def __init__(self, ctx, name, blocks):
        self._c, self._name, self._b = ctx, name, blocks

    def put(self, a, upload=None):
        """an input (None: None, nothing reserved). upload: the array the device form uploads in its place"""
        if a is None:
            return None
        if self._b is None:
            return _Staged(a.ctypes.data, a, a.shape, a.dtype)
        a = a if upload is None else upload
        return _Staged(self._b.up(a), a, a.shape, a.dtype)

    def new(self, shape, dtype, dev_shape=None, nbytes=None, fill=None):
        """an output of that shape and dtype. dev_shape: what the device form reserves and hands back where that is another shape; nbytes: the size of its block where
        that is not the array's; fill: the byte its block holds before the call (the host form's array then holds zeros)"""
        if self._b is None:
            arr = np.empty(shape, dtype) if fill is None else np.zeros(shape, dtype)
            return _Staged(arr.ctypes.data, arr, arr.shape, arr.dtype)
        shape = tuple(shape if dev_shape is None else dev_shape)
        if fill is not None:
            return _Staged(self._b.up(np.full(shape, fill, dtype)), None, shape, dtype)
        return _Staged(self._b.new(math.prod(shape) * np.dtype(dtype).itemsize if nbytes is None else nbytes), None, shape, dtype)

    def over(self, out, inp):
        """where a call writes under an alias or in-place switch: `out`, or in the device form the block of the input `inp` (None: the switch is off). The host form
        has no such switch and writes `out`"""
        return out if self._b is None or inp is None else inp

    @staticmethod
    def list(staged):
        """a void*[K] of staged arrays (None entries: NULL; None: NULL)"""
        return None if staged is None else (C.c_void_p * max(len(staged), 1))(*[None if s is None else s.ptr for s in staged])

    def call(self, *args, host_only=()):
        """nct_<name>[_dev](ctx, *args), a staged array as its pointer; host_only: what only the host form takes behind them"""
        fn = getattr(self._c._l, "nct_" + self._name + ("_dev" if self._b is not None else ""))
        self._c._chk(fn(self._c._h, *[a.ptr if isinstance(a, _Staged) else a for a in args + (tuple(host_only) if self._b is None else ())]))

    def get(self, s):
        """a staged array after the call: the host array, or the download of its block (None: None)"""
        if s is None:
            return None
        return s.arr if self._b is None else self._c.dev_download(s.ptr, s.shape, s.dtype)


class Context:
    """One context per GPU / process (include/nct.h: not thread-safe)."""

    def __init__(self, device=0):
        self._l = lib()
        h = C.c_void_p()
        rc = self._l.nct_create(device, C.byref(h))
        if rc != 0:
            raise NctError(rc, self._l.nct_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._l.nct_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise NctError(rc, self._l.nct_last_error(self._h).decode())

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._chk(self._l.nct_device_name(self._h, buf, 256))
        return buf.value.decode()

    def counter(self, which):
        """nct_ctx_counter: CTR_ARENA_BYTES, CTR_S1_HUB_BLOCKS_L0 + level"""
        v = C.c_int64(0)
        self._chk(self._l.nct_ctx_counter(self._h, which, C.byref(v)))
        return v.value

    def synchronize(self):
        self._chk(self._l.nct_synchronize(self._h))

    # ---- N1
    def feat_normalize(self, src_chw, want_resp=False):
        src = np.ascontiguousarray(src_chw, np.float32)
        Cc, H, W = src.shape
        dst = np.empty_like(src)
        resp = np.empty((H, W), np.float32) if want_resp else None
        self._chk(self._l.nct_feat_normalize(self._h, src, dst, _ptr(resp), Cc, H, W))
        return (dst, resp) if want_resp else dst

    # ---- N2
    def nnf_init(self, ah, aw, bh, bw):
        nnf = np.empty((ah, aw), np.uint32)
        self._chk(self._l.nct_nnf_init(self._h, nnf, ah, aw, bh, bw))
        return nnf

    def nnf_upsample(self, nnf_half, ah, aw, bh, bw):
        half = np.ascontiguousarray(nnf_half, np.uint32)
        nnf = np.empty((ah, aw), np.uint32)
        self._chk(self._l.nct_nnf_upsample(self._h, half, nnf, ah, aw, bh, bw, half.shape[0], half.shape[1]))
        return nnf

    # ---- P1
    def patchmatch(self, a_chw, b_chw, nnf, iters=10, rs_max=32, seed=0, patch=3):
        a = np.ascontiguousarray(a_chw, np.float32)
        b = np.ascontiguousarray(b_chw, np.float32)
        Cc, ah, aw = a.shape
        _, bh, bw = b.shape
        nnf = np.array(nnf, np.uint32, order="C", copy=True).reshape(ah, aw)
        dist = np.empty((ah, aw), np.float32)
        self._chk(self._l.nct_patchmatch(self._h, a, b, Cc, ah, aw, bh, bw, patch, iters, rs_max, seed, nnf, dist))
        return nnf, dist

    # ---- B2
    def bds_vote_features(self, ann, bnn, pin_chw, w_coh=1.0, w_comp=2.0, patch=3, want_pw=False):
        pin = np.ascontiguousarray(pin_chw, np.float32)
        Cc, bh, bw = pin.shape
        ann = np.ascontiguousarray(ann, np.uint32)
        bnn = np.ascontiguousarray(bnn, np.uint32)
        ah, aw = ann.shape
        pout = np.empty((Cc, ah, aw), np.float32)
        pw = np.empty((ah, aw), np.float32) if want_pw else None
        self._chk(self._l.nct_bds_vote_features(self._h, ann, bnn, pin, pout, _ptr(pw), Cc, ah, aw, bh, bw, patch, w_coh, w_comp))
        return (pout, pw) if want_pw else pout

    def feature_distance(self, a_chw, b_chw):
        a = np.ascontiguousarray(a_chw, np.float32)
        b = np.ascontiguousarray(b_chw, np.float32)
        Cc, H, W = a.shape
        err = np.empty((H, W), np.float32)
        self._chk(self._l.nct_feature_distance(self._h, a, b, err, Cc, H, W))
        return err

    # ---- B1
    def bds_vote_image(self, a_bgr, b_bgr, ann, bnn, w_coh=1.0, w_comp=2.0, patch=3):
        a = np.ascontiguousarray(a_bgr, np.uint8)
        b = np.ascontiguousarray(b_bgr, np.uint8)
        ah, aw = a.shape[:2]
        bh, bw = b.shape[:2]
        out = np.empty((ah, aw, 3), np.uint8)
        self._chk(self._l.nct_bds_vote_image(self._h, a, ah, aw, b, bh, bw, np.ascontiguousarray(ann, np.uint32),
                                             np.ascontiguousarray(bnn, np.uint32), patch, w_coh, w_comp, out))
        return out

    # ---- V1 / V2
    VGG_CIN = [3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512]
    VGG_COUT = [64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512]
    VGG_NAMES = ["conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv3_4",
                 "conv4_1", "conv4_2", "conv4_3", "conv4_4", "conv5_1", "conv5_2", "conv5_3", "conv5_4"]
    TAP_C = [64, 128, 256, 512, 512]

    def vgg19_load_caffemodel(self, path):
        self._chk(self._l.nct_vgg19_load_caffemodel(self._h, os.fsencode(path)))

    # ---- device-pointer seams (nct_dev.cpp): buffers are plain integers (device addresses); nothing synchronises until dev_download / synchronize
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self._l.nct_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, p):
        self._chk(self._l.nct_dev_free(self._h, p))

    @contextlib.contextmanager
    def blocks(self, held=()):
        """the arena blocks of a piece of work -> a _Blocks: up(array) uploads into a new block, new(nbytes) takes one, free(p) gives one back early. On every way
        out the stream is synchronised, then the blocks still held go back. held: blocks taken before (dev_upload, dev_alloc), which go back with them"""
        b = _Blocks(self)
        b.held.extend(held)
        try:
            yield b
        finally:
            self.synchronize()
            for p in b.held:
                self.dev_free(p)

    _blocks = blocks                                               # the name blocks(held) had while it was private: callers written against it keep working

    @contextlib.contextmanager
    def _seam(self, name, dev):
        """one call of the seam nct_<name> in its host form or (dev) in its device form on arena blocks -> a _Seam; the blocks go back as blocks() gives them back"""
        with (self.blocks() if dev else contextlib.nullcontext()) as b:
            yield _Seam(self, name, b)

    def dev_upload(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.dev_alloc(a.nbytes)
        self._chk(self._l.nct_dev_upload(self._h, p, a.ctypes.data, a.nbytes))
        return p

    def dev_download(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self._chk(self._l.nct_dev_download(self._h, out.ctypes.data, p, out.nbytes))
        return out

    def dev_call(self, name, *args):
        """nct_<name>_dev(ctx, *args)"""
        self._chk(getattr(self._l, "nct_" + name + "_dev")(self._h, *args))

    def vgg19_load_model(self, model):
        """model: a Model (nct_model_parse_caffemodel) — upload the host copy to this context's GPU"""
        self._chk(self._l.nct_vgg19_load_model(self._h, model._m))

    def vgg19_share_weights(self, other):
        """use `other`'s device copy of the weights (same GPU): no parse, no upload, no second copy"""
        self._chk(self._l.nct_vgg19_share_weights(self._h, other._h))

    def vgg19_weights_info(self):
        i, b, n = C.c_uint64(), C.c_size_t(), C.c_int()
        self._chk(self._l.nct_vgg19_weights_info(self._h, C.byref(i), C.byref(b), C.byref(n)))
        return {"id": i.value, "bytes": b.value, "sharers": n.value}

    def vgg19_check_prototxt(self, path):
        self._chk(self._l.nct_vgg19_check_prototxt(self._h, os.fsencode(path)))

    def vgg19_load_raw(self, weights, biases):
        ws = [np.ascontiguousarray(w, np.float32) for w in weights]
        bs = [np.ascontiguousarray(b, np.float32) for b in biases]
        n = len(ws)
        wp = (C.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        self._chk(self._l.nct_vgg19_load_raw(self._h, wp, bp, n))

    def vgg19_features(self, bgr, deepest_tap=5, stride=None):
        """-> list of `deepest_tap` CHW fp32 arrays (tap 1 = conv1_1 … tap 5 = conv5_1). stride: the image is handed over in a buffer with that many bytes from
        one row to the next (>= 3 w; the bytes between rows are 0xFF) instead of packed."""
        img = np.ascontiguousarray(bgr, np.uint8)
        h, w = img.shape[:2]
        if stride is not None and stride >= 3 * w:
            buf = np.full((h, stride), 0xFF, np.uint8)
            buf[:, :3 * w] = img.reshape(h, 3 * w)
            img = buf
        outs = [np.empty((self.TAP_C[t],) + hw, np.float32) for t, hw in enumerate(_level_dims(h, w)[::-1][:deepest_tap])]
        ptrs = (C.c_void_p * 5)(*([o.ctypes.data for o in outs] + [None] * (5 - deepest_tap)))
        dims = np.zeros(15, np.int32)
        self._chk(self._l.nct_vgg19_features(self._h, img, h, w, w * 3 if stride is None else stride, deepest_tap, ptrs, _ptr(dims)))
        for t, o in enumerate(outs):
            assert tuple(dims[3 * t:3 * t + 3]) == o.shape
        return outs

    def conv3x3_relu(self, x_chw, weights, bias, relu=True):
        x = np.ascontiguousarray(x_chw, np.float32)
        w = np.ascontiguousarray(weights, np.float32)
        b = np.ascontiguousarray(bias, np.float32)
        cin, H, W = x.shape
        cout = w.shape[0]
        out = np.empty((cout, H, W), np.float32)
        self._chk(self._l.nct_conv3x3_relu(self._h, x, cin, H, W, w, b, cout, out, 1 if relu else 0))
        return out

    def maxpool2x2(self, x_chw):
        x = np.ascontiguousarray(x_chw, np.float32)
        c, H, W = x.shape
        out = np.empty((c, (H - 1) // 2 + 1, (W - 1) // 2 + 1), np.float32)
        self._chk(self._l.nct_maxpool2x2(self._h, x, c, H, W, out))
        return out

    # ---- colour stage
    def bgr2lab(self, bgr):
        a = np.ascontiguousarray(bgr, np.uint8)
        out = np.empty_like(a)
        self._chk(self._l.nct_bgr2lab_u8(self._h, a.reshape(-1, 3), a.size // 3, out.reshape(-1, 3)))
        return out

    def lab2bgr(self, lab, form=None):
        a = np.ascontiguousarray(lab, np.uint8)
        out = np.empty_like(a)
        if form is None:
            self._chk(self._l.nct_lab2bgr_u8(self._h, a.reshape(-1, 3), a.size // 3, out.reshape(-1, 3)))
        else:
            self._chk(self._l.nct_lab2bgr_u8_form(self._h, a.reshape(-1, 3), a.size // 3, out.reshape(-1, 3), form))
        return out

    def resize_u8c3(self, img, dh, dw):
        a = np.ascontiguousarray(img, np.uint8)
        out = np.empty((dh, dw, 3), np.uint8)
        self._chk(self._l.nct_resize_u8c3(self._h, a, a.shape[0], a.shape[1], out, dh, dw))
        return out

    def resize_f64c3(self, img, dh, dw):
        a = np.ascontiguousarray(img, np.float64)
        out = np.empty((dh, dw, 3), np.float64)
        self._chk(self._l.nct_resize_f64c3(self._h, a, a.shape[0], a.shape[1], out, dh, dw))
        return out

    def cluster_features(self, feat_chw, K=10, iters=11, seed=1):
        f = np.ascontiguousarray(feat_chw, np.float32)
        Cc, h, w = f.shape
        labels = np.empty((h, w), np.int32)
        nl = C.c_int()
        self._chk(self._l.nct_cluster_features(self._h, f, Cc, h, w, K, iters, seed, labels.reshape(-1), C.byref(nl)))
        return labels, nl.value

    def knn_graph(self, lab_u8, labels, nlabels, samples, k=8):
        lab = np.ascontiguousarray(lab_u8, np.uint8)
        h, w = lab.shape[:2]
        lb = np.ascontiguousarray(labels, np.int32)
        ids = np.empty((h * w, k), np.int32)
        ws = np.empty((h * w, k), np.float64)
        self._chk(self._l.nct_knn_graph(self._h, lab, h, w, lb.reshape(-1), lb.shape[0], lb.shape[1], nlabels, samples, k, ids.reshape(-1), ws.reshape(-1)))
        return ids, ws

    def local_color_transfer(self, err, s_level, g_level, s_full, knn_id, knn_w, layer, params=None, want_stages=False):
        err = np.ascontiguousarray(err, np.float32)
        h, w = err.shape
        s_full = np.ascontiguousarray(s_full, np.uint8)
        H, W = s_full.shape[:2]
        prm = params or Params.default()
        out = np.empty((H, W, 3), np.uint8)
        st, keep = None, {}
        if want_stages:
            keep = {"ab_local": np.empty((2, h * w, 3)), "ab_nonlocal": np.empty((2, h * w, 3)), "ab_up": np.empty((2, H * W, 3)),
                    "roughness": np.empty(H * W), "ab_wls": np.empty((2, H * W, 3)), "cg_iters": np.zeros(3, np.int32), "wls_iters": np.zeros(6, np.int32)}
            st = ColorStages(*[keep[k].ctypes.data for k in ("ab_local", "ab_nonlocal", "ab_up", "roughness", "ab_wls", "cg_iters", "wls_iters")])
        self._chk(self._l.nct_local_color_transfer(self._h, err.reshape(-1), np.ascontiguousarray(s_level, np.uint8).reshape(-1, 3),
                                                   np.ascontiguousarray(g_level, np.uint8).reshape(-1, 3), s_full.reshape(-1, 3),
                                                   np.ascontiguousarray(knn_id, np.int32).reshape(-1), np.ascontiguousarray(knn_w, np.float64).reshape(-1),
                                                   layer, h, w, H, W, C.addressof(prm), out.reshape(-1, 3), C.addressof(st) if st else None))
        return (out, keep) if want_stages else out

    # ---- per-pair hot loop
    def _process(self, name, src_bgr, args, params, want_timing):
        """what every process_* method does around its own C entry point `name`(ctx, source, h, w, *args, params, result, timing): the source and the result, the
        defaults, the timing. An array among args is an image or a mask (None: none) and goes over as the declared argument type takes it"""
        s = np.ascontiguousarray(src_bgr, np.uint8)
        prm = params or Params.default()
        out = np.empty_like(s)
        tm = PairTiming() if want_timing else None
        fn = getattr(self._l, name)
        call = [self._h, s, s.shape[0], s.shape[1], *args, C.addressof(prm), out, C.addressof(tm) if tm is not None else None]
        self._chk(fn(*[(a if t is _u8p else a.ctypes.data) if isinstance(a, np.ndarray) else a for a, t in zip(call, fn.argtypes)]))
        return (out, tm.as_dict()) if want_timing else out

    @staticmethod
    def _image(bgr):
        """-> the image as contiguous bytes, its height, its width: the three arguments an image takes"""
        a = np.ascontiguousarray(bgr, np.uint8)
        return a, a.shape[0], a.shape[1]

    def process_pair(self, src_bgr, ref_bgr, params=None, want_timing=False):
        return self._process("nct_process_pair", src_bgr, self._image(ref_bgr), params, want_timing)

    def process_pair_fullres(self, src_bgr, ref_bgr, max_side=1000, params=None, want_timing=False, finish=0):
        """nct_process_pair_fullres: the pair runs at working_size(..., max_side), the last level finishes on the original source (result: src's size).
        finish: FINISH_EXACT (0) that entry point; anything else goes through nct_process_pair_fullres_finish (FINISH_UPSAMPLE: SPEC §6.8)"""
        if finish == FINISH_EXACT:
            return self._process("nct_process_pair_fullres", src_bgr, [*self._image(ref_bgr), max_side], params, want_timing)
        return self._process("nct_process_pair_fullres_finish", src_bgr, [*self._image(ref_bgr), max_side, int(finish)], params, want_timing)

    def color_finish_upsample(self, ab_wls, h, w, s_full, params=None, *, dev=False):
        """nct_color_finish_upsample[_dev] (SPEC §6.8): ab_wls ([2][h*w][3], the working-size finish's S2 output) upsampled and applied to s_full (H x W x 3 BGR)"""
        return self._finish(ab_wls, None, h, w, s_full, params, dev)

    def color_finish_guided(self, ab_wls, lab_work, h, w, s_full, sigma=None, params=None, *, dev=False):
        """nct_color_finish_guided[_dev] (SPEC §6.10): the upsampling finish with joint-bilateral weights; lab_work (h x w x 3): the 8-bit Lab image of the working-size
        source; sigma None = the library's default"""
        return self._finish(ab_wls, np.ascontiguousarray(lab_work, np.uint8), h, w, s_full, params, dev, _guided_params(sigma))

    def color_finish_upsample_region(self, ab_wls, h, w, s_full, mask, protect=None, params=None, *, dev=False):
        """nct_color_finish_upsample_region[_dev] (SPEC §6.13 rule 4): color_finish_upsample with §6.11's compose in its pass; mask [H, W] bytes of s_full, None: the
        unmasked call"""
        return self._finish(ab_wls, None, h, w, s_full, params, dev, None, (mask, protect))

    def color_finish_guided_region(self, ab_wls, lab_work, h, w, s_full, mask, protect=None, sigma=None, params=None, *, dev=False):
        """nct_color_finish_guided_region[_dev] (SPEC §6.13 rule 4): color_finish_guided with §6.11's compose in its pass"""
        return self._finish(ab_wls, np.ascontiguousarray(lab_work, np.uint8), h, w, s_full, params, dev, _guided_params(sigma), (mask, protect))

    def _finish(self, ab_wls, lw, h, w, s_full, params, dev, gp=None, region=None):
        """the four upsampling finish seams: lw / gp None = the plain finish, else the guided one; region None = the unmasked entry point, else (mask, protect) of the
        masked one"""
        a = np.ascontiguousarray(ab_wls, np.float64).reshape(-1)
        assert a.size == 6 * h * w and (lw is None or lw.size == 3 * h * w)
        s_full = np.ascontiguousarray(s_full, np.uint8)
        H, W = s_full.shape[:2]
        name = "color_finish_" + ("upsample" if lw is None else "guided") + ("" if region is None else "_region")
        mask, protect = region or (None, None)
        m = None if mask is None else _mask_arg(mask, s_full.shape, name)
        prm, rg = params or Params.default(), _region_params(protect)
        tail = ([] if region is None else [C.addressof(rg)]) + ([] if lw is None else [C.addressof(gp)]) + [C.addressof(prm)]
        with self._seam(name, dev) as s:
            ins = [s.put(a)] + ([] if lw is None else [s.put(lw)])
            src, out = s.put(s_full), s.new((H, W, 3), np.uint8)
            s.call(*ins, h, w, src, H, W, *([] if region is None else [s.put(m)]), *tail, out)         # the mask goes up behind the output block
            return s.get(out)

    def set_finish_guided(self, sigma):
        """nct_set_finish_guided: a sigma turns the guided modifier of the upsampling finish on for this context, None turns it off (the default)"""
        if sigma is None:
            self._chk(self._l.nct_set_finish_guided(self._h, None))
        else:
            gp = _guided_params(sigma)
            self._chk(self._l.nct_set_finish_guided(self._h, C.addressof(gp)))

    def color_finish(self, ab, h, w, work_h, work_w, s_full, params=None, want_stages=False):
        """nct_color_finish: U1 / roughness / S2 / A1 of ab ([2][h*w][3], S1's ab_nonlocal) onto s_full (H x W x 3 BGR) in a pyramid of working size work_h x work_w"""
        a = np.ascontiguousarray(ab, np.float64).reshape(-1)
        assert a.size == 6 * h * w
        s_full = np.ascontiguousarray(s_full, np.uint8)
        H, W = s_full.shape[:2]
        prm = params or Params.default()
        out = np.empty((H, W, 3), np.uint8)
        st, keep = None, {}
        if want_stages:
            keep = {"ab_up": np.empty((2, H * W, 3)), "roughness": np.empty(H * W), "ab_wls": np.empty((2, H * W, 3)), "wls_iters": np.zeros(6, np.int32)}
            st = ColorStages(None, None, keep["ab_up"].ctypes.data, keep["roughness"].ctypes.data, keep["ab_wls"].ctypes.data, None, keep["wls_iters"].ctypes.data)
        self._chk(self._l.nct_color_finish(self._h, a, h, w, work_h, work_w, s_full.reshape(-1, 3), H, W, C.addressof(prm), out.reshape(-1, 3),
                                           C.addressof(st) if st else None))
        return (out, keep) if want_stages else out

    # ---- several references (SPEC §6.2)
    @staticmethod
    def _ref_list(refs):
        """-> (K, contiguous arrays, void*[K], int[K] heights, int[K] widths); K and null entries are checked by the library, not here"""
        arrs = [None if r is None else np.ascontiguousarray(r, np.uint8) for r in refs]
        K = len(arrs)
        ptrs = (C.c_void_p * max(K, 1))(*[None if a is None else a.ctypes.data for a in arrs])
        hs = (C.c_int * max(K, 1))(*[0 if a is None else a.shape[0] for a in arrs])
        ws = (C.c_int * max(K, 1))(*[0 if a is None else a.shape[1] for a in arrs])
        return K, arrs, ptrs, hs, ws

    def select_reference(self, errs, guides=None, *, dev=False):
        """nct_select_reference[_dev]: K error maps (h x w fp32) and, optionally, K guidance images (h x w x 3) -> (label, merged guide or None, merged err)"""
        es = [np.ascontiguousarray(e, np.float32) for e in errs]
        gs = None if guides is None else [np.ascontiguousarray(g, np.uint8) for g in guides]
        K = len(es)
        h, w = es[0].shape if K else (1, 1)
        with self._seam("select_reference", dev) as s:
            ep, gp = [s.put(e) for e in es], None if gs is None else [s.put(g) for g in gs]
            label, gout, eout = s.new((h, w), np.uint8), None if gs is None else s.new((h, w, 3), np.uint8), s.new((h, w), np.float32)
            s.call(s.list(ep), s.list(gp), K, h, w, label, gout, eout)
            return s.get(label), s.get(gout), s.get(eout)

    def process_multi(self, src_bgr, refs_bgr, params=None, want_timing=False):
        """nct_process_multi: one source, a list of references -> the result at the source's size"""
        K, keep, ptrs, hs, ws = self._ref_list(refs_bgr)
        return self._process("nct_process_multi", src_bgr, [K, ptrs, hs, ws], params, want_timing)

    def multi_upload(self, src_bgr, refs_bgr):
        s = np.ascontiguousarray(src_bgr, np.uint8)
        K, keep, ptrs, hs, ws = self._ref_list(refs_bgr)
        self._pair_shape = s.shape
        self._chk(self._l.nct_multi_upload(self._h, s.reshape(-1, 3), s.shape[0], s.shape[1], K, ptrs, hs, ws))
        self._multi_shapes = [a.shape for a in keep]

    def multi_run(self, params=None, want_timing=False):
        prm = params or Params.default()
        tm = PairTiming() if want_timing else None
        self._chk(self._l.nct_multi_run(self._h, C.addressof(prm), C.addressof(tm) if tm is not None else None))
        return tm.as_dict() if want_timing else None

    def multi_run_levels(self, params=None):
        """nct_multi_run_levels on the uploaded list -> dict: per reference and level "ann", "bnn", "annd", "bnnd", "ref_guide", "ref_err" ([k][l]); per level the merged
        "label", "guide", "err", "result" ([l]); "labels" (k-means), "timing". Level 0 = coarsest."""
        keep, structs = _multi_reports(_grids(self._pair_shape, self._multi_shapes), 5)
        return self._run_call("nct_multi_run_levels", params, keep, *structs)

    def _run_call(self, name, params, keep, *structs):
        """a run of the uploaded images through the library's `name`(ctx, params, timing, *structs) -> keep, "timing" added"""
        prm = params or Params.default()
        tm = PairTiming()
        self._chk(getattr(self._l, name)(self._h, C.addressof(prm), C.addressof(tm), *[C.addressof(st) for st in structs]))
        keep["timing"] = tm.as_dict()
        return keep

    # ---- reference region masks (SPEC §6.12)
    def region_pull(self, q_mask, ann, bnn, w_coh=1.0, w_comp=2.0, *, dev=False):
        """nct_region_pull[_dev] (SPEC §6.12 rule 2): q_mask [bh, bw] bytes, ann [ah, aw] and bnn [bh, bw] NNF words -> the pulled mask [ah, aw]"""
        q, a, b = np.ascontiguousarray(q_mask, np.uint8), np.ascontiguousarray(ann, np.uint32), np.ascontiguousarray(bnn, np.uint32)
        if q.shape != b.shape:
            raise NctError(-2, f"region_pull: mask is {q.shape}, bnn {b.shape}")
        with self._seam("region_pull", dev) as s:
            qs, as_, bs, out = s.put(q), s.put(a), s.put(b), s.new(a.shape, np.uint8)
            s.call(qs, q.shape[0], q.shape[1], as_, bs, a.shape[0], a.shape[1], w_coh, w_comp, out)
            return s.get(out)

    def pair_set_ref_region(self, k, mask, protect=None):
        """nct_pair_set_ref_region on the uploaded references: reference k's mask [rh, rw] bytes, or None to remove it; protect None leaves the run's protect as it is"""
        rg = None if protect is None else _region_params(protect)
        if mask is None:
            self._chk(self._l.nct_pair_set_ref_region(self._h, int(k), None, None if rg is None else C.addressof(rg)))
            return
        shapes = getattr(self, "_multi_shapes", [])
        m = np.ascontiguousarray(mask, np.uint8)
        if 0 <= k < len(shapes):                        # the library refuses a k out of range
            m = _mask_arg(mask, shapes[k], "pair_set_ref_region")
        self._chk(self._l.nct_pair_set_ref_region(self._h, int(k), m.ctypes.data, None if rg is None else C.addressof(rg)))

    def multi_run_ref_region_levels(self, params=None):
        """nct_multi_run_ref_region_levels on the uploaded, masked list -> multi_run_levels' dict plus "ref_mask" and "pulled" ([k][l]; unmasked references stay zero),
        "mask" [h, w], "mask_full" [H, W] and "ab_mix" [2, h*w, 3] per level"""
        keep, structs = _multi_reports(_grids(self._pair_shape, self._multi_shapes), 5, RefRegionLevels)
        return self._run_call("nct_multi_run_ref_region_levels", params, keep, *structs)

    def process_pair_ref_region(self, src_bgr, src_mask, ref_bgr, ref_mask, protect=None, params=None, want_timing=False):
        """nct_process_pair_ref_region: process_pair with a mask on the source ([h, w] of the source) and / or on the reference ([rh, rw]); both None: process_pair"""
        r, rh, rw = self._image(ref_bgr)
        m = None if src_mask is None else _mask_arg(src_mask, np.shape(src_bgr), "process_pair_ref_region")
        q = None if ref_mask is None else _mask_arg(ref_mask, r.shape, "process_pair_ref_region (reference)")
        rg = _region_params(protect)
        self._pair_shape = np.shape(src_bgr); self._multi_shapes = [r.shape]
        return self._process("nct_process_pair_ref_region", src_bgr, [m, r, rh, rw, q, C.addressof(rg)], params, want_timing)

    def process_multi_ref_region(self, src_bgr, src_mask, refs_bgr, ref_masks, protect=None, params=None, want_timing=False):
        """nct_process_multi_ref_region: process_multi with a mask on the source and / or on some references (ref_masks: None, or a list with None entries)"""
        K, keep, ptrs, hs, ws = self._ref_list(refs_bgr)
        m = None if src_mask is None else _mask_arg(src_mask, np.shape(src_bgr), "process_multi_ref_region")
        qs, qp = None, None
        if ref_masks is not None:
            if len(ref_masks) != K:
                raise NctError(-2, f"process_multi_ref_region: {len(ref_masks)} masks for {K} references")
            qs = [None if q is None else _mask_arg(q, keep[k].shape, "process_multi_ref_region (reference %d)" % k) for k, q in enumerate(ref_masks)]
            qp = (C.c_void_p * max(K, 1))(*[None if q is None else q.ctypes.data for q in qs])
        rg = _region_params(protect)
        self._pair_shape = np.shape(src_bgr); self._multi_shapes = [a.shape for a in keep]
        return self._process("nct_process_multi_ref_region", src_bgr, [m, K, ptrs, hs, ws, qp, C.addressof(rg)], params, want_timing)

    def process_pair_fullres_ref_region(self, src_bgr, mask0, ref_bgr, ref_mask0, max_side=1000, protect=None, params=None, want_timing=False):
        """nct_process_pair_fullres_ref_region (SPEC §6.12 rule 5): both masks at their images' original sizes; the exact finish"""
        r, rh, rw = self._image(ref_bgr)
        m = None if mask0 is None else _mask_arg(mask0, np.shape(src_bgr), "process_pair_fullres_ref_region")
        q = None if ref_mask0 is None else _mask_arg(ref_mask0, r.shape, "process_pair_fullres_ref_region (reference)")
        rg = _region_params(protect)
        return self._process("nct_process_pair_fullres_ref_region", src_bgr, [m, r, rh, rw, q, max_side, C.addressof(rg)], params, want_timing)

    # ---- frame sequences (SPEC §6.3)
    _seq = None                                                   # the open sequence (a _Seq), None when there is none

    def _seq_begun(self, src_shape, refs, levels, max_side=None, finish=None):
        """the record of the sequence a seq_begin* call has opened; max_side and finish: of a full-resolution sequence"""
        arrive, ref_arrive = tuple(src_shape[:2]), [r.shape[:2] for r in refs]
        if max_side is None:
            self._seq = _Seq(arrive, ref_arrive, arrive, ref_arrive, levels, None)
        else:
            self._seq = _Seq(arrive, ref_arrive, working_size(int(arrive[0]), int(arrive[1]), max_side), [working_size(h, w, max_side) for h, w in ref_arrive], levels, int(finish))

    def _seq_record(self, what, begin):
        """-> the open sequence's record; `what` needs one"""
        if self._seq is None:
            raise NctError(-5, "%s: no sequence is open (%s first)" % (what, begin))
        return self._seq

    def _seq_grids(self):
        """the grids of the open sequence's reports: they live at the working size, but the last level run of an exact full-resolution finish targets the arriving size"""
        q = self._seq
        return _grids(q.work, q.ref_work, [q.arrive if (q.finish == FINISH_EXACT and l == q.levels - 1) else q.work for l in range(5)])

    def _seq_params(self, params, tau, sigma, hold=None):
        """-> Params, SeqParams and SeqHold (None: NULL) of a seq_begin* call, the library's defaults where an argument is left out"""
        prm = params or Params.default()
        sp = SeqParams.default()
        if tau is not None:
            sp.tau = tau
        if sigma is not None:
            sp.sigma = sigma
        hp = None
        if hold is not None:
            hp = SeqHold(); hp.hold = hold
        return prm, sp, hp

    def seq_begin(self, ref_bgr, src_shape, params=None, tau=None, sigma=None):
        """nct_seq_begin: prepare the reference once for frames of src_shape[:2]; tau / sigma default to nct_seq_params_default (0.7, 10.0)"""
        r = np.ascontiguousarray(ref_bgr, np.uint8)
        prm, sp, _ = self._seq_params(params, tau, sigma)
        self._chk(self._l.nct_seq_begin(self._h, r.reshape(-1, 3), r.shape[0], r.shape[1], int(src_shape[0]), int(src_shape[1]), C.addressof(prm), C.addressof(sp)))
        self._seq_begun(src_shape, [r], prm.levels)

    def seq_begin_fullres(self, ref_bgr, src_shape, max_side=1000, finish=0, params=None, tau=None, sigma=None):
        """nct_seq_begin_fullres (SPEC §6.9): frames of src_shape[:2] and the reference arrive at their original size and are shrunk to working_size(..., max_side) on
        the device; every frame call then takes and returns originals. finish: FINISH_EXACT or FINISH_UPSAMPLE"""
        r = np.ascontiguousarray(ref_bgr, np.uint8)
        prm, sp, _ = self._seq_params(params, tau, sigma)
        self._chk(self._l.nct_seq_begin_fullres(self._h, r.reshape(-1, 3), r.shape[0], r.shape[1], int(src_shape[0]), int(src_shape[1]), int(max_side), int(finish),
                                                C.addressof(prm), C.addressof(sp)))
        self._seq_begun(src_shape, [r], prm.levels, max_side, finish)

    # ---- sequences over several references (SPEC §6.18)
    def seq_begin_multi(self, refs_bgr, src_shape, params=None, tau=None, sigma=None, hold=None):
        """nct_seq_begin_multi: prepare a list of references once for frames of src_shape[:2]; hold None passes NULL (nct_seq_hold_default)"""
        K, keep, ptrs, hs, ws = self._ref_list(refs_bgr)
        prm, sp, hp = self._seq_params(params, tau, sigma, hold)
        self._chk(self._l.nct_seq_begin_multi(self._h, K, ptrs, hs, ws, int(src_shape[0]), int(src_shape[1]), C.addressof(prm), C.addressof(sp),
                                              None if hp is None else C.addressof(hp)))
        self._seq_begun(src_shape, keep, prm.levels)

    def seq_begin_multi_fullres(self, refs_bgr, src_shape, max_side=1000, finish=0, params=None, tau=None, sigma=None, hold=None):
        """nct_seq_begin_multi_fullres: seq_begin_fullres over a list of references"""
        K, keep, ptrs, hs, ws = self._ref_list(refs_bgr)
        prm, sp, hp = self._seq_params(params, tau, sigma, hold)
        self._chk(self._l.nct_seq_begin_multi_fullres(self._h, K, ptrs, hs, ws, int(src_shape[0]), int(src_shape[1]), int(max_side), int(finish), C.addressof(prm),
                                                      C.addressof(sp), None if hp is None else C.addressof(hp)))
        self._seq_begun(src_shape, keep, prm.levels, max_side, finish)

    def _seq_frame_call(self, name, s, keep, *structs):
        """the frame s (_seq_frame_arg has checked it) through the library's `name`(ctx, frame, result, timing, *structs), a struct None as NULL -> (result, keep with
        "timing" added). What the structs point at stays with the caller until this returns"""
        out = np.empty_like(s)
        tm = PairTiming()
        self._chk(getattr(self._l, name)(self._h, s.reshape(-1, 3), out.reshape(-1, 3), C.addressof(tm), *[None if st is None else C.addressof(st) for st in structs]))
        keep["timing"] = tm.as_dict()
        return out, keep

    def _seq_multi_reports(self, *more):
        """what the full frames over several references report: MultiLevels at the working size (a full-resolution sequence reports no "result"), SeqLevels and
        SeqHoldLevels for the levels that run, then the structs in `more` -> _reports' pair"""
        q = self._seq
        keep, structs = _multi_reports(self._seq_grids(), q.levels, SeqLevels, SeqHoldLevels, *more)
        if q.finish is not None:
            del keep["result"]
            structs[0].result = (C.c_void_p * 5)()
        return keep, structs

    def seq_frame_multi_levels(self, src_bgr, want_color=True):
        """nct_seq_frame_multi[_stage]_levels -> (result, dict): multi_run_levels' lists at the working size ("ann" … "ref_err" as [k][l]; "label", "guide", "err", "result"
        as [l]; "labels"), seq_frame_levels' "ab_blend", "tau_map" and "motion" per level that ran, the held selection's "free_label" and "margin" per level that ran, with
        want_color "color" (a dict per level that ran, as seq_frame_levels reports it) and "timing". A full-resolution sequence reports neither "result" nor "color"."""
        s, q = self._seq_frame_arg(src_bgr, "seq_frame_multi_levels"), self._seq_record("seq_frame_multi_levels", "seq_begin_multi")
        self._pair_shape, self._multi_shapes = q.work + (3,), [r + (3,) for r in q.ref_work]
        keep, (lv, sl, hl) = self._seq_multi_reports()
        if not want_color or q.finish is not None:
            return self._seq_frame_call("nct_seq_frame_multi_levels", s, keep, lv, sl, hl)
        keep["color"], cptr, stages = _color_stages(self._seq_grids(), q.levels, q.levels)
        return self._seq_frame_call("nct_seq_frame_multi_stage_levels", s, keep, lv, cptr, sl, hl)

    def select_reference_hold(self, errs, guides, prev_label, lab, lab_prev, field=None, hold=0.0, sigma=10.0, *, dev=False, want=("label", "guide", "err", "free_label", "margin")):
        """nct_select_reference_hold[_dev]: K error maps [h, w] fp32, K guidance images [h, w, 3] (or None), the kept labels [h, w], the two frames' 8-bit Lab level
        images, a field int16 [h, w, 2] or None -> dict of the outputs named in `want` (the others are passed as NULL)"""
        es = [np.ascontiguousarray(e, np.float32) for e in errs]
        gs = None if guides is None else [np.ascontiguousarray(g, np.uint8) for g in guides]
        K = len(es)
        h, w = es[0].shape if K else (1, 1)
        pl, l1, l0 = np.ascontiguousarray(prev_label, np.uint8), np.ascontiguousarray(lab, np.uint8), np.ascontiguousarray(lab_prev, np.uint8)
        f = None if field is None else np.ascontiguousarray(field, np.int16)
        want = [k for k in want if not (k == "guide" and gs is None)]
        spec = {"label": ((h, w), np.uint8), "guide": ((h, w, 3), np.uint8), "err": ((h, w), np.float32), "free_label": ((h, w), np.uint8), "margin": ((h, w), np.float64)}
        with self._seam("select_reference_hold", dev) as s:
            ep, gp = [s.put(e) for e in es], None if gs is None else [s.put(g) for g in gs]
            ins = [s.put(pl), s.put(l1), s.put(l0), s.put(f)]
            outs = {k: s.new(*spec[k]) for k in want}
            s.call(s.list(ep), s.list(gp), K, h, w, *ins, float(hold), float(sigma), *[outs.get(k) for k in ("label", "guide", "err", "free_label", "margin")])
            return {k: s.get(outs[k]) for k in want}

    def seq_frame(self, src_bgr, want_timing=False):
        s = self._seq_frame_arg(src_bgr, "seq_frame")
        out = np.empty_like(s)
        tm = PairTiming() if want_timing else None
        self._chk(self._l.nct_seq_frame(self._h, s.reshape(-1, 3), out.reshape(-1, 3), C.addressof(tm) if tm is not None else None))
        return (out, tm.as_dict()) if want_timing else out

    def seq_set_region(self, mask, protect=None):
        """nct_seq_set_region (SPEC §6.13) on the open sequence: mask [h, w] bytes at the size frames arrive, or None to remove it. Sticky until replaced or removed"""
        if mask is None:
            self._chk(self._l.nct_seq_set_region(self._h, None, None))
            return
        rg = _region_params(protect)
        if self._seq is None:                                  # no open sequence: the library refuses; the mask is never read
            m = np.ascontiguousarray(mask, np.uint8)
        else:
            m = _mask_arg(mask, self._seq.arrive, "seq_set_region")
        self._chk(self._l.nct_seq_set_region(self._h, m.ctypes.data, C.addressof(rg)))

    # ---- reference region masks in sequences (SPEC §6.19)
    def seq_set_ref_region(self, k, mask, protect=None):
        """nct_seq_set_ref_region on the open sequence: reference k's mask [rh, rw] bytes at the size that reference arrived, or None to remove it. Sticky until replaced or
        removed; protect None leaves the run's protect as it is"""
        rg = None if protect is None else _region_params(protect)
        if mask is None:
            self._chk(self._l.nct_seq_set_ref_region(self._h, int(k), None, None if rg is None else C.addressof(rg)))
            return
        shapes = [] if self._seq is None else self._seq.ref_arrive
        m = np.ascontiguousarray(mask, np.uint8)
        if 0 <= k < len(shapes):                        # the library refuses a k out of range and a call without a sequence; the mask is then never read
            m = _mask_arg(mask, shapes[k], "seq_set_ref_region")
        self._chk(self._l.nct_seq_set_ref_region(self._h, int(k), m.ctypes.data, None if rg is None else C.addressof(rg)))

    def seq_pull_hold(self, pulled, label, prev, lab, lab_prev, field=None, src_mask=None, tau=0.7, sigma=10.0, *, dev=False, alias=False, want=("p", "m", "p_free"), shape=None):
        """nct_seq_pull_hold[_dev]: K pulled masks [h, w] bytes (None entries: 255), the label map [h, w] (None with one reference), the kept map, the two frames' 8-bit
        Lab level images, a field int16 [h, w, 2] or None, the source level mask or None -> dict of the outputs named in `want` ("p" is always written). shape: the
        grid, where no array gives it. alias (device form): p_out is prev's block, which is an error"""
        ps = [None if q is None else np.ascontiguousarray(q, np.uint8) for q in pulled]
        K = len(ps)
        pv, l1, l0 = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(lab, np.uint8), np.ascontiguousarray(lab_prev, np.uint8)
        h, w = shape if shape is not None else pv.shape[:2]
        lb = None if label is None else np.ascontiguousarray(label, np.uint8)
        f = None if field is None else np.ascontiguousarray(field, np.int16)
        ms = None if src_mask is None else np.ascontiguousarray(src_mask, np.uint8)
        order = ("p", "m", "p_free")
        want = [k for k in order if k in want or k == "p"]
        with self._seam("seq_pull_hold", dev) as s:
            pp = [s.put(q) for q in ps]
            lbs, fs, mss = s.put(lb), s.put(f), s.put(ms)
            pvs, l1s, l0s = s.put(pv), s.put(l1), s.put(l0)
            outs = {k: s.new((int(h), int(w)), np.uint8) for k in want}
            p_out = s.over(outs["p"], pvs if alias else None)
            s.call(s.list(pp), K, lbs, pvs, l1s, l0s, fs, mss, int(h), int(w), float(tau), float(sigma), p_out, outs.get("m"), outs.get("p_free"))
            return {k: s.get(outs[k]) for k in want}

    def seq_frame_ref_region_levels(self, src_bgr):
        """nct_seq_frame_ref_region_levels -> (result, dict): seq_frame_multi_levels' dict without "color", plus per level that ran "ref_mask" and "pulled" ([k][l]; unmasked
        references stay zero), "mask" (M_l), "mask_full" (F_l at the size the level's finish targets), "ab_mix", "p_free" (P_l) and "p_held" (P'_t)"""
        s, q = self._seq_frame_arg(src_bgr, "seq_frame_ref_region_levels"), self._seq_record("seq_frame_ref_region_levels", "seq_begin")
        self._pair_shape, self._multi_shapes = q.work + (3,), [r + (3,) for r in q.ref_work]
        keep, (lv, sl, hl, rl, pl) = self._seq_multi_reports(RefRegionLevels, SeqPullLevels)
        return self._seq_frame_call("nct_seq_frame_ref_region_levels", s, keep, lv, None, sl, hl, rl, pl)

    def seq_frame_propagate_ref_region_levels(self, src_bgr):
        """nct_seq_frame_propagate_ref_region_levels -> (result, dict): seq_frame_propagate_levels' dict plus "p_held" per level that ran and, for the last level run only
        (zeros elsewhere), "mask", "mask_full" and "ab_mix" maps"""
        s, q = self._seq_frame_arg(src_bgr, "seq_frame_propagate_ref_region_levels"), self._seq_record("seq_frame_propagate_ref_region_levels", "seq_begin")
        g = self._seq_grids()
        keep, structs = _reports(g, q.levels, SeqLevels, RefRegionLevels, SeqPullLevels)
        keep["dims"] = g.src
        return self._seq_frame_call("nct_seq_frame_propagate_ref_region_levels", s, keep, *structs)

    # ---- region tracking (SPEC §6.14)
    def seq_matte_warp(self, mask, field, *, dev=False, alias=False):
        """nct_seq_matte_warp[_dev] (SPEC §6.14 rule 1): mask [H, W] bytes, field int16 [h, w, 2] of (my, mx) on a level grid -> the matte read at p + d(p), d the field
        interpolated at p in target pixels. alias (device form): into the matte's block, which is an error"""
        m = np.ascontiguousarray(mask, np.uint8)
        f = np.ascontiguousarray(field, np.int16)
        if m.ndim != 2 or f.ndim != 3 or f.shape[2] != 2:
            raise NctError(-2, "seq_matte_warp: mask must be [H, W] bytes and field [h, w, 2] int16")
        (H, W), (h, w) = m.shape, f.shape[:2]
        with self._seam("seq_matte_warp", dev) as s:
            ms, fs, out = s.put(m), s.put(f), s.new((H, W), np.uint8)
            s.call(ms, H, W, fs, h, w, s.over(out, ms if alias else None))
            return s.get(out)

    # ---- correspondence carry (SPEC §6.23)
    def seq_set_carry(self, on=True, iters=-1):
        """nct_seq_set_carry: from the next full frame on the open sequence starts every level's PatchMatch from the merge of its ordinary start field and the kept
        fields of the last frame (True), or as it always did (False). iters: PatchMatch iterations of a frame that merged, -1 = the sequence's pm_iters"""
        self._chk(self._l.nct_seq_set_carry(self._h, int(on), int(iters)))

    def seq_get_carry(self, k=0, l=0):
        """nct_seq_get_carry -> (ann [ah_l, aw_l], bnn [bh_l, bw_l]) uint32: the kept fields of reference k at level run l as the last frame left them"""
        q = self._seq_record("seq_get_carry", "seq_begin")
        g = self._seq_grids()
        if not (0 <= k < len(g.ref) and 0 <= l < q.levels):      # the library refuses; nothing is written
            self._chk(self._l.nct_seq_get_carry(self._h, int(k), int(l), None, None))
        ann, bnn = np.empty(g.src[l], np.uint32), np.empty(g.ref[k][l], np.uint32)
        self._chk(self._l.nct_seq_get_carry(self._h, int(k), int(l), ann.ctypes.data, bnn.ctypes.data))
        return ann, bnn

    def nnf_carry(self, nnf_prev, field, *, dev=False, alias=False):
        """nct_nnf_carry[_dev] (SPEC §6.23 rule 3): nnf_prev [h, w] uint32, field int16 [h, w, 2] of (my, mx) -> nnf_prev read at the clamped p + m(p). alias (device
        form): into nnf_prev's block, which is an error"""
        f = np.ascontiguousarray(field, np.int16)
        h, w = f.shape[:2]
        a = np.ascontiguousarray(nnf_prev, np.uint32)
        assert a.size == h * w and f.size == 2 * h * w
        with self._seam("nnf_carry", dev) as s:
            as_, fs, out = s.put(a), s.put(f), s.new((h, w), np.uint32)
            s.call(as_, h, w, fs, s.over(out, as_ if alias else None))
            return s.get(out)

    def nnf_forward_map(self, field, *, dev=False, alias=False):
        """nct_nnf_forward_map[_dev] (SPEC §6.23 rule 4): field int16 [h, w, 2] -> F [h, w] uint32. alias (device form): into the field's block, which is an error"""
        f = np.ascontiguousarray(field, np.int16)
        h, w = f.shape[:2]
        with self._seam("nnf_forward_map", dev) as s:
            fs, out = s.put(f), s.new((h, w), np.uint32)
            s.call(fs, h, w, s.over(out, fs if alias else None))
            return s.get(out)

    def nnf_remap(self, bnn_prev, fwd, *, dev=False, alias=False):
        """nct_nnf_remap[_dev] (SPEC §6.23 rule 4): bnn_prev [bh, bw] uint32, fwd [h, w] uint32 -> fwd read at bnn_prev's words. alias (device form): into bnn_prev's
        block, which is an error"""
        b, fw = np.ascontiguousarray(bnn_prev, np.uint32), np.ascontiguousarray(fwd, np.uint32)
        (bh, bw), (h, w) = b.shape, fw.shape
        with self._seam("nnf_remap", dev) as s:
            bs, fs, out = s.put(b), s.put(fw), s.new((bh, bw), np.uint32)
            s.call(bs, bh, bw, fs, h, w, s.over(out, bs if alias else None))
            return s.get(out)

    def nnf_merge(self, a_chw, b_chw, z, c, *, dev=False, alias=False, want_dist=True, patch=3):
        """nct_nnf_merge[_dev] (SPEC §6.23 rule 6, one direction): normalised features a [C, ah, aw] and b [C, bh, bw] (the device form uploads them channel-last), the
        ordinary start field z and the moved kept field c, [ah, aw] uint32 -> (start, d_z, d_c), or start alone. alias (device form): into z's block, which is an error"""
        a, b = np.ascontiguousarray(a_chw, np.float32), np.ascontiguousarray(b_chw, np.float32)
        (Cc, ah, aw), (_, bh, bw) = a.shape, b.shape
        z_, c_ = np.ascontiguousarray(z, np.uint32).reshape(ah, aw), np.ascontiguousarray(c, np.uint32).reshape(ah, aw)
        hwc = lambda m: np.ascontiguousarray(m.reshape(m.shape[0], -1).T)
        with self._seam("nnf_merge", dev) as s:
            as_, bs = s.put(a, upload=hwc(a)), s.put(b, upload=hwc(b))
            zs, cs, out = s.put(z_), s.put(c_), s.new((ah, aw), np.uint32)
            dz, dc = (s.new((ah, aw), np.float32), s.new((ah, aw), np.float32)) if want_dist else (None, None)
            s.call(as_, bs, Cc, ah, aw, bh, bw, int(patch), zs, cs, s.over(out, zs if alias else None), dz, dc)
            return (s.get(out), s.get(dz), s.get(dc)) if want_dist else s.get(out)

    def seq_set_region_tracking(self, on):
        """nct_seq_set_region_tracking: from the next frame on the open sequence's matte follows the motion field (True) or stays sticky (False)"""
        self._chk(self._l.nct_seq_set_region_tracking(self._h, int(on)))

    def seq_get_region(self):
        """nct_seq_get_region -> (the matte in force at the size frames arrive, its age in frames)"""
        out = np.zeros(self._seq.arrive if self._seq is not None else (1, 1), np.uint8)      # no open sequence: the library refuses; nothing is written
        age = C.c_int(-1)
        self._chk(self._l.nct_seq_get_region(self._h, out.ctypes.data, C.addressof(age)))
        return out, age.value

    # ---- matte snapping (SPEC §6.15)
    def region_snap(self, mask, lab, radius=None, sigma=None, binary=None, *, dev=False, alias=None):
        """nct_region_snap[_dev] (SPEC §6.15 rule 1): mask [H, W] bytes, lab [H, W, 3] the same frame in 8-bit Lab -> the matte re-fitted to the guide's edges; a
        parameter left None keeps its default (radius 3, sigma 10, binary 1). alias "mask" / "lab" (device form): into that input's block, which is an error"""
        m, g = np.ascontiguousarray(mask, np.uint8), np.ascontiguousarray(lab, np.uint8)
        if m.ndim != 2 or g.shape != m.shape + (3,):
            raise NctError(-2, "region_snap: mask must be [H, W] bytes and lab [H, W, 3] bytes")
        H, W = m.shape
        sp = _snap_params(radius, sigma, binary)
        with self._seam("region_snap", dev) as s:
            ms, gs, out = s.put(m), s.put(g), s.new((H, W), np.uint8)
            s.call(ms, gs, H, W, C.addressof(sp), s.over(out, {None: None, "mask": ms, "lab": gs}[alias]))
            return s.get(out)

    def seq_set_region_snap(self, on=True, radius=None, sigma=None, binary=None):
        """nct_seq_set_region_snap: from the next frame on the open sequence's tracked matte is snapped to its frame's edges behind the carry (on; a parameter left
        None keeps its default), or not (on false: NULL)"""
        if not on:
            self._chk(self._l.nct_seq_set_region_snap(self._h, None))
            return
        sp = _snap_params(radius, sigma, binary)
        self._chk(self._l.nct_seq_set_region_snap(self._h, C.addressof(sp)))

    # ---- region selection from strokes (SPEC §6.16)
    def region_select(self, src_bgr, strokes, params=None, want_stages=False, *, dev=False):
        """nct_region_select[_dev] (SPEC §6.16): src_bgr [h, w, 3], strokes [h, w] bytes (STROKE_IN inside, STROKE_OUT outside, else unmarked) -> the matte [h, w];
        params: region_select_params(...) or None for the defaults. want_stages (host form only; refused with dev): -> (matte, {"q" [cells, C] int16, "cell", "score"
        [h_t, w_t], "up" [h, w]})"""
        s_, t = np.ascontiguousarray(src_bgr, np.uint8), np.ascontiguousarray(strokes, np.uint8)
        if s_.ndim != 3 or s_.shape[2] != 3 or t.shape != s_.shape[:2]:
            raise NctError(-2, "region_select: src_bgr must be [h, w, 3] bytes and strokes [h, w] bytes")
        if want_stages and dev:
            raise NctError(-2, "region_select: want_stages is host-only (nct_region_select_dev reports no stages)")
        h, w = t.shape
        st, cs = None, None
        if want_stages:
            tap = params.tap if params is not None else RegionSelectParams.default().tap
            if not 1 <= tap <= 5:                                  # the library refuses; the stage arrays are never written
                tap = 1
            ht, wt = ((h - 1) >> (tap - 1)) + 1, ((w - 1) >> (tap - 1)) + 1
            st = {"q": np.zeros((ht * wt, self.TAP_C[tap - 1]), np.int16), "cell": np.zeros((ht, wt), np.uint8), "score": np.zeros((ht, wt), np.uint8),
                  "up": np.zeros((h, w), np.uint8)}
            cs = RegionSelectStages(*[st[k].ctypes.data for k in ("q", "cell", "score", "up")])
        with self._seam("region_select", dev) as s:
            ss, ts, out = s.put(s_), s.put(t), s.new((h, w), np.uint8)
            s.call(ss, h, w, ts, C.addressof(params) if params is not None else None, out, host_only=[C.addressof(cs) if cs is not None else None])
            return (s.get(out), st) if want_stages else s.get(out)

    def feat_quantize(self, src_chw, *, dev=False):
        """nct_feat_quantize[_dev] (SPEC §6.16 rule 2): CHW fp32 features -> [H*W, C] int16 rows rint(N1(F) * 32767); the device form takes the map channel-last"""
        src = np.ascontiguousarray(src_chw, np.float32)
        Cc, H, W = src.shape
        with self._seam("feat_quantize", dev) as s:
            ins, out = s.put(src, upload=np.ascontiguousarray(src.reshape(Cc, H * W).T)), s.new((H * W, Cc), np.int16)
            s.call(ins, out, Cc, H, W)
            return s.get(out)

    def region_score(self, q, seeds_in, seeds_out=None, sharpness=1024, floor_permille=700, *, dev=False):
        """nct_region_score[_dev] (SPEC §6.16 rule 4 without the seed-cell overwrite): q [cells, C], seeds_in [n_in, C], seeds_out [n_out, C] or None, int16 -> [cells] bytes"""
        qq, si = np.ascontiguousarray(q, np.int16), np.ascontiguousarray(seeds_in, np.int16)
        so = None if seeds_out is None or len(seeds_out) == 0 else np.ascontiguousarray(seeds_out, np.int16)
        cells, Cc = qq.shape
        n_in, n_out = si.shape[0], 0 if so is None else so.shape[0]
        with self._seam("region_score", dev) as s:
            qs, sis, sos, out = s.put(qq), s.put(si), s.put(so), s.new((cells,), np.uint8)
            s.call(qs, cells, Cc, sis, n_in, sos, n_out, int(sharpness), int(floor_permille), out)
            return s.get(out)

    # ---- reference libraries (SPEC §6.21)
    def feat_quantize8(self, src_chw, center=None, *, dev=False):
        """nct_feat_quantize8[_dev] (SPEC §6.21 rule D2): CHW fp32 features, center [C] or None -> [H*W, C] int8 rows rint(N1(F - center) * 127); the device form takes
        the map channel-last"""
        src = np.ascontiguousarray(src_chw, np.float32)
        mu = None if center is None else np.ascontiguousarray(center, np.float32)
        Cc, H, W = src.shape
        with self._seam("feat_quantize8", dev) as s:
            ins, mus, out = s.put(src, upload=np.ascontiguousarray(src.reshape(Cc, H * W).T)), s.put(mu), s.new((H * W, Cc), np.int8)
            s.call(ins, mus, out, Cc, H, W)
            return s.get(out)

    def descriptor_match(self, a, entries, *, dev=False):
        """nct_descriptor_match[_dev] (SPEC §6.21 rule D3): a [na, C] int8 and a list of entries [n_k, C] int8 -> (fwd [N], bwd [N]) int64"""
        aa = np.ascontiguousarray(a, np.int8)
        ents = [np.ascontiguousarray(e, np.int8) for e in entries]
        na, Cc = aa.shape
        rows = np.ascontiguousarray(np.concatenate(ents, axis=0)) if ents else np.zeros((0, Cc), np.int8)
        offs = np.concatenate([[0], np.cumsum([e.shape[0] for e in ents])]).astype(np.int32)
        with self._seam("descriptor_match", dev) as s:
            as_, rs, f, b = s.put(aa), s.put(rows), s.new((len(ents),), np.int64), s.new((len(ents),), np.int64)
            s.call(as_, na, Cc, rs, offs, len(ents), f, b)
            return s.get(f), s.get(b)

    def reflib_rank(self, reflib, src_bgr, wf=None, wb=None):
        """nct_reflib_rank (SPEC §6.21): src_bgr [h, w, 3] against every entry of the RefLib -> (order [N] int32, key, fwd, bwd [N] int64); wf / wb None: 1, 1"""
        img = np.ascontiguousarray(src_bgr, np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise NctError(-2, "reflib_rank: src_bgr must be [h, w, 3] bytes")
        N = reflib.info()[2]
        prm = None
        if wf is not None or wb is not None:
            prm = RefLibParams.default()
            prm.wf, prm.wb = int(prm.wf if wf is None else wf), int(prm.wb if wb is None else wb)
        order, key, fwd, bwd = np.zeros(max(N, 1), np.int32), np.zeros(max(N, 1), np.int64), np.zeros(max(N, 1), np.int64), np.zeros(max(N, 1), np.int64)
        self._chk(self._l.nct_reflib_rank(self._h, reflib._m, img.ctypes.data, img.shape[0], img.shape[1], C.addressof(prm) if prm is not None else None,
                                          order.ctypes.data, key.ctypes.data, fwd.ctypes.data, bwd.ctypes.data))
        return order[:N], key[:N], fwd[:N], bwd[:N]

    def reflib_release(self):
        """nct_reflib_release: the device copy of the library last ranked against goes back to the arena"""
        self._chk(self._l.nct_reflib_release(self._h))

    def descriptor_match_bench(self, d_a, na, Cc, d_rows, offsets, d_fwd, d_bwd, reps=20):
        """nct_descriptor_match_bench on device pointers (offsets: a host int32 array) -> the mean device time of one match in ms"""
        offs = np.ascontiguousarray(offsets, np.int32)
        ms = C.c_float()
        self._chk(self._l.nct_descriptor_match_bench(self._h, d_a, na, Cc, d_rows, offs.ctypes.data, offs.size - 1, d_fwd, d_bwd, reps, C.byref(ms)))
        return ms.value

    def pair_select_region(self, strokes, params=None, protect=None):
        """nct_pair_select_region: region_select on the uploaded source, then pair_set_region with the matte, which stays on the device"""
        t = _mask_arg(strokes, self._pair_shape, "pair_select_region")
        rg = _region_params(protect)
        self._chk(self._l.nct_pair_select_region(self._h, t.ctypes.data, C.addressof(params) if params is not None else None, C.addressof(rg)))

    def seq_select_region(self, frame_bgr, strokes, params=None, protect=None):
        """nct_seq_select_region on the open sequence: region_select on frame_bgr (a frame of the sequence's size), then seq_set_region with the matte"""
        f, t = np.ascontiguousarray(frame_bgr, np.uint8), np.ascontiguousarray(strokes, np.uint8)
        if self._seq is not None and (tuple(f.shape[:2]) != self._seq.arrive or t.shape != self._seq.arrive):
            raise NctError(-2, "seq_select_region: the frame and the strokes must have the size the sequence was begun for")
        rg = _region_params(protect)
        self._chk(self._l.nct_seq_select_region(self._h, f.ctypes.data, t.ctypes.data, C.addressof(params) if params is not None else None, C.addressof(rg)))

    # ---- region models (SPEC §6.17)
    def region_model_fit(self, src_bgr, strokes, params=None):
        """nct_region_model_fit: §6.16 rules 1 to 3 on src_bgr [h, w, 3] and strokes [h, w] -> a RegionModel of the kept seed rows (of params only tap and max_seeds act)"""
        s, t = np.ascontiguousarray(src_bgr, np.uint8), np.ascontiguousarray(strokes, np.uint8)
        if s.ndim != 3 or s.shape[2] != 3 or t.shape != s.shape[:2]:
            raise NctError(-2, "region_model_fit: src_bgr must be [h, w, 3] bytes and strokes [h, w] bytes")
        m = C.c_void_p()
        self._chk(self._l.nct_region_model_fit(self._h, s.ctypes.data, t.shape[0], t.shape[1], t.ctypes.data, C.addressof(params) if params is not None else None, C.byref(m)))
        return RegionModel(_handle=m)

    def region_model_add(self, model, src_bgr, strokes, params=None):
        """nct_region_model_add: another image's kept seed rows appended to the model"""
        s, t = np.ascontiguousarray(src_bgr, np.uint8), np.ascontiguousarray(strokes, np.uint8)
        if s.ndim != 3 or s.shape[2] != 3 or t.shape != s.shape[:2]:
            raise NctError(-2, "region_model_add: src_bgr must be [h, w, 3] bytes and strokes [h, w] bytes")
        self._chk(self._l.nct_region_model_add(self._h, model._m, s.ctypes.data, t.shape[0], t.shape[1], t.ctypes.data, C.addressof(params) if params is not None else None))

    def region_refind(self, score, shape, prior=None, margin=32, *, dev=False, alias=None):
        """nct_region_refind[_dev] (SPEC §6.17 rules R1 to R3): score [ht, wt] bytes on the tap grid, shape (H, W), prior [H, W] bytes or None -> the matte [H, W].
        alias "score" / "prior" (device form): into that input's block, which is an error"""
        m = np.ascontiguousarray(score, np.uint8)
        pr = None if prior is None else np.ascontiguousarray(prior, np.uint8)
        H, W = int(shape[0]), int(shape[1])
        if m.ndim != 2 or (pr is not None and pr.shape != (H, W)):
            raise NctError(-2, "region_refind: score must be [ht, wt] bytes and prior [H, W] bytes or None")
        ht, wt = m.shape
        with self._seam("region_refind", dev) as s:
            ms, ps = s.put(m), s.put(pr)
            out = s.new((max(H, 1), max(W, 1)), np.uint8, dev_shape=(H, W), nbytes=max(H * W, max(m.size, 1)))      # a refused size never reaches the host array
            s.call(ms, ht, wt, ps, H, W, int(margin), s.over(out, {None: None, "score": ms, "prior": ps or ms}[alias]))
            return s.get(out)

    def region_model_apply(self, model, src_bgr, prior=None, params=None, want_stages=False, *, dev=False):
        """nct_region_model_apply[_dev] (SPEC §6.17 rules A1 to A4): the model's object re-found on src_bgr [h, w, 3] -> the matte [h, w]; prior [h, w] bytes or None;
        params: region_refind_params(...) or None for the defaults. want_stages (host form only; refused with dev): -> (matte, {"q" [cells, C] int16, "score"
        [h_t, w_t], "refound" [h, w]})"""
        s_ = np.ascontiguousarray(src_bgr, np.uint8)
        pr = None if prior is None else np.ascontiguousarray(prior, np.uint8)
        if s_.ndim != 3 or s_.shape[2] != 3 or (pr is not None and pr.shape != s_.shape[:2]):
            raise NctError(-2, "region_model_apply: src_bgr must be [h, w, 3] bytes and prior [h, w] bytes or None")
        if want_stages and dev:
            raise NctError(-2, "region_model_apply: want_stages is host-only (nct_region_model_apply_dev reports no stages)")
        h, w = s_.shape[:2]
        st, cs = None, None
        if want_stages:
            tap, Cc, _, _ = model.info()
            ht, wt = ((h - 1) >> (tap - 1)) + 1, ((w - 1) >> (tap - 1)) + 1
            st = {"q": np.zeros((ht * wt, Cc), np.int16), "score": np.zeros((ht, wt), np.uint8), "refound": np.zeros((h, w), np.uint8)}
            cs = RegionApplyStages(*[st[k].ctypes.data for k in ("q", "score", "refound")])
        with self._seam("region_model_apply", dev) as s:
            ss, ps, out = s.put(s_), s.put(pr), s.new((h, w), np.uint8)
            s.call(model._m, ss, h, w, ps, C.addressof(params) if params is not None else None, out, host_only=[C.addressof(cs) if cs is not None else None])
            return (s.get(out), st) if want_stages else s.get(out)

    def pair_apply_region_model(self, model, params=None, protect=None):
        """nct_pair_apply_region_model: region_model_apply without a prior on the uploaded source, then pair_set_region with the matte, which stays on the device"""
        rg = _region_params(protect)
        self._chk(self._l.nct_pair_apply_region_model(self._h, model._m, C.addressof(params) if params is not None else None, C.addressof(rg)))

    def seq_set_region_model(self, model, params=None, protect=None):
        """nct_seq_set_region_model on the open sequence (SPEC §6.17 rules S1 to S6): from the next full frame on the model's object is re-found on every full frame,
        with the carried matte as the prior; model None removes it"""
        if model is None:
            self._chk(self._l.nct_seq_set_region_model(self._h, None, None, None))
            return
        rg = _region_params(protect)
        self._chk(self._l.nct_seq_set_region_model(self._h, model._m, C.addressof(params) if params is not None else None, C.addressof(rg)))

    def seq_frame_region_levels(self, src_bgr, want_color=True, want_levels=None):
        """nct_seq_frame_region_levels -> seq_frame_levels' (result, dict) plus per level that ran "ab_mix" (the mixed map the finish read, [2, h*w, 3]) and "mask" (M_l [h, w])"""
        return self.seq_frame_levels(src_bgr, want_color, want_levels, _region=True)

    def seq_frame_propagate_region_levels(self, src_bgr):
        """nct_seq_frame_propagate_region_levels -> seq_frame_propagate_levels' (result, dict) plus "ab_mix" and "mask" per level that ran: the last level run's mixed map
        (zeros elsewhere) and the level masks that were built (that level and finer; zeros elsewhere)"""
        return self.seq_frame_propagate_levels(src_bgr, _region=True)

    def _seq_region_call(self, name, s, keep, g, levels, region, *first):
        """the end of the two single-reference frame reports: SeqLevels for the levels that run and, with region, RegionLevels go behind the structs in `first`.
        nct_region_levels takes a mask for all five levels; "mask" reports those that ran"""
        more, structs = _reports(g, levels, SeqLevels, *([RegionLevels] if region else []))
        keep.update(more)
        out, keep = self._seq_frame_call(name, s, keep, *first, *structs)
        if region:
            keep["mask"] = keep["mask"][:levels]
        return out, keep

    def seq_frame_levels(self, src_bgr, want_color=True, want_levels=None, _region=False):
        """nct_seq_frame_levels -> (result, dict): pair_run_levels' per-level lists ("ann" … "result", with want_color "color" and "labels"), plus "ab_blend" and "tau_map"
        per level that ran (X'_t [2, h*w, 3] and tau_p [h, w]; a frame without a blend reports X_t and zeros), "motion" (SPEC §6.4: the level's field, int16 [h, w, 2] of
        (my, mx); zeros without motion or without a blend) and "timing"."""
        s, q = self._seq_frame_arg(src_bgr, "seq_frame_levels"), self._seq_record("seq_frame_levels", "seq_begin")
        # a full-resolution sequence (SPEC §6.9 rule 5) reports the working-size maps through "ab_blend" / "tau_map" / "motion" only: nct_pair_levels stays NULL
        # unless want_levels forces it (which the library refuses)
        if want_levels is None:
            want_levels = q.finish is None
        g = self._seq_grids()
        keep, lv, hold = _pair_report(g, q.levels, want_color and want_levels)
        if not want_levels:
            keep, lv = {"dims": keep["dims"]}, None
        return self._seq_region_call("nct_seq_frame_region_levels" if _region else "nct_seq_frame_levels", s, keep, g, q.levels, _region, lv)

    def _seq_frame_arg(self, src_bgr, what):
        s = np.ascontiguousarray(src_bgr, np.uint8)
        if self._seq is not None and tuple(s.shape[:2]) != self._seq.arrive:
            raise NctError(-2, "%s: the frame is %dx%d, the sequence was begun for %dx%d" % (what, s.shape[1], s.shape[0], self._seq.arrive[1], self._seq.arrive[0]))
        return s

    def seq_frame_propagate(self, src_bgr, want_timing=False):
        """nct_seq_frame_propagate (SPEC §6.5): the frame takes the previous frame's coefficients through the motion field and runs the last level's finish only"""
        s = self._seq_frame_arg(src_bgr, "seq_frame_propagate")
        out = np.empty_like(s)
        tm = PairTiming() if want_timing else None
        self._chk(self._l.nct_seq_frame_propagate(self._h, s.reshape(-1, 3), out.reshape(-1, 3), C.addressof(tm) if tm is not None else None))
        return (out, tm.as_dict()) if want_timing else out

    def seq_frame_propagate_levels(self, src_bgr, _region=False):
        """nct_seq_frame_propagate_levels -> (result, dict): per level that ran "ab_blend" (X'_t [2, h*w, 3]), "motion" (int16 [h, w, 2]; zeros with motion off) and
        "tau_map" (1.0 everywhere), plus "timing" and "dims" (the source's level grids)"""
        s, q = self._seq_frame_arg(src_bgr, "seq_frame_propagate_levels"), self._seq
        g = self._seq_grids() if q is not None else _grids(s.shape, [])        # no open sequence: the library refuses; no level is reported
        name = "nct_seq_frame_propagate_region_levels" if _region else "nct_seq_frame_propagate_levels"
        return self._seq_region_call(name, s, {"dims": g.src}, g, q.levels if q is not None else 0, _region)

    def seq_warp(self, x_prev, field, *, dev=False, alias=False):
        """nct_seq_warp[_dev] (SPEC §6.5 rule 3): x_prev [2, h*w, 3] doubles, field int16 [h, w, 2] of (my, mx) -> x_prev read at p + m(p), the 64-bit words copied.
        alias (device form): into x_prev's block, which is an error"""
        f = np.ascontiguousarray(field, np.int16)
        h, w = f.shape[:2]
        a = np.ascontiguousarray(x_prev, np.float64).reshape(-1)
        assert a.size == 6 * h * w and f.size == 2 * h * w
        with self._seam("seq_warp", dev) as s:
            xs, fs, out = s.put(a), s.put(f), s.new((2, h * w, 3), np.float64)
            s.call(xs, h, w, fs, s.over(out, xs if alias else None))
            return s.get(out)


    # ---- adaptive key frames (SPEC §6.7)
    def seq_change(self, lab, lab_prev, field=None, threshold=24, *, dev=False):
        """nct_seq_change[_dev] (SPEC §6.7 rule 1): lab / lab_prev h x w x 3 8-bit Lab, field None or int16 [h, w, 2] of (my, mx) -> {"sad", "changed", "pixels"}.
        The device form's record block holds 0xff bytes before the call"""
        a = np.ascontiguousarray(lab, np.uint8)
        b = np.ascontiguousarray(lab_prev, np.uint8)
        h, w = a.shape[:2]
        f = None if field is None else np.ascontiguousarray(field, np.int16)
        assert b.shape == a.shape and (f is None or f.size == 2 * h * w)
        with self._seam("seq_change", dev) as s:
            as_, bs, fs, rec = s.put(a), s.put(b), s.put(f), s.new((C.sizeof(SeqChange),), np.uint8, fill=0xff)
            s.call(as_, bs, h, w, fs, int(threshold), rec)
            return SeqChange.from_buffer_copy(s.get(rec).tobytes()).as_dict()

    def seq_probe(self, src_bgr, auto=None):
        """nct_seq_probe (SPEC §6.7 rule 2): the decision the frame would get on the open sequence, nothing changed -> dict (SeqDecision.as_dict); auto: a SeqAuto or
        None = the defaults"""
        s = self._seq_frame_arg(src_bgr, "seq_probe")
        d = SeqDecision()
        self._chk(self._l.nct_seq_probe(self._h, s.ctypes.data, C.addressof(auto) if auto is not None else None, C.addressof(d)))
        return d.as_dict()

    def seq_frame_auto(self, src_bgr, auto=None, want_timing=False):
        """nct_seq_frame_auto (SPEC §6.7 rule 4): probe, decide, run the frame -> (result, decision dict[, timing dict])"""
        s = self._seq_frame_arg(src_bgr, "seq_frame_auto")
        out = np.empty_like(s)
        d = SeqDecision()
        tm = PairTiming() if want_timing else None
        self._chk(self._l.nct_seq_frame_auto(self._h, s.ctypes.data, out.ctypes.data, C.addressof(tm) if tm is not None else None,
                                             C.addressof(auto) if auto is not None else None, C.addressof(d)))
        return (out, d.as_dict(), tm.as_dict()) if want_timing else (out, d.as_dict())

    # ---- 3D colour look-up tables (SPEC §6.6)
    def lut_fit(self, src, res, size=None, lam=None, want_stages=False, *, dev=False):
        """nct_lut_fit[_dev]: source and result images (any shape [..., 3], uint8 BGR) -> table float32 [N, N, N, 3] (+ {"weight", "resid", "disp"}); size / lam left
        out are nct_lut_params_default's"""
        return self._lut_fit("lut_fit", src, res, None, size, lam, want_stages, dev)

    def lut_fit_masked(self, src, res, mask, size=None, lam=None, want_stages=False, *, dev=False):
        """nct_lut_fit_masked[_dev] (SPEC §6.11 rule 7): lut_fit over the pixels with mask >= 128 (mask None: lut_fit)"""
        return self._lut_fit("lut_fit_masked", src, res, mask, size, lam, want_stages, dev)

    def _lut_fit(self, name, src, res, mask, size, lam, want_stages, dev):
        """the two fits: the unmasked one is the masked one without a mask, through its own entry point"""
        s_, r = np.ascontiguousarray(src, np.uint8).reshape(-1, 3), np.ascontiguousarray(res, np.uint8).reshape(-1, 3)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert s_.shape == r.shape and (m is None or len(m) == len(s_))
        prm = _lut_params(size, lam)
        n = prm.size
        N = n if 0 < n <= 65 else 1                                # a refused size never reaches the host arrays; the device form asks for it as it stands
        with self._seam(name, dev) as s:
            ss, rs = s.put(s_), s.put(r)
            lut, st, cs = self._lut_outputs(s, N, n)
            ms = [s.put(m)] if name == "lut_fit_masked" else []        # the mask goes up behind the four output blocks
            s.call(ss, rs, *ms, len(s_), C.addressof(prm), lut, C.addressof(cs) if want_stages else None)
            return (s.get(lut), {k: s.get(v) for k, v in st.items()}) if want_stages else s.get(lut)

    @staticmethod
    def _lut_outputs(s, N, n):
        """what a fit or a solve writes, staged on the seam s: the table, the three stages by name and the struct of their pointers. N: the side of the host arrays,
        n: the side the device form reserves"""
        spec = {"weight": ((), np.uint64), "resid": ((3,), np.int64), "disp": ((3,), np.float64)}
        lut = s.new((N, N, N, 3), np.float32, dev_shape=(n, n, n, 3))
        st = {k: s.new((N ** 3,) + tail, t, dev_shape=(n ** 3,) + tail) for k, (tail, t) in spec.items()}
        return lut, st, LutStages(*(st[k].ptr for k in ("weight", "resid", "disp")))

    def lut_apply(self, lut, img, *, dev=False, in_place=False):
        """nct_lut_apply[_dev]: table [N, N, N, 3] float32 on an image [..., 3] uint8 BGR -> the image of the same shape. in_place (device form): the output over
        the input"""
        return self._lut_apply("lut_apply", np.uint8, lut, img, dev, in_place)

    def lut_apply_u16(self, lut, img16, *, dev=False, in_place=False):
        """nct_lut_apply_u16[_dev] (SPEC §6.20): lut_apply on an image [..., 3] uint16 BGR, a value v standing for the grey level v / 257"""
        return self._lut_apply("lut_apply_u16", np.uint16, lut, img16, dev, in_place)

    def _lut_apply(self, name, dtype, lut, img, dev, in_place):
        """the two applies: the same call on pixels of another depth"""
        t = np.ascontiguousarray(lut, np.float32)
        a = np.ascontiguousarray(img, dtype)
        with self._seam(name, dev) as s:
            ts, as_, out = s.put(t), s.put(a), s.new(a.shape, dtype)
            dst = s.over(out, as_ if in_place else None)
            s.call(ts, t.shape[0], as_, a.size // 3, dst)
            return s.get(dst)

    # ---- the shot accumulator (SPEC §6.20): one table over many frames
    def lut_accum_begin(self, size):
        """nct_lut_accum_begin: open the context's accumulator for tables of that lattice size"""
        self._chk(self._l.nct_lut_accum_begin(self._h, int(size)))
        self._lut_accum_size = int(size)

    def lut_accum_add(self, src, res, mask=None, *, dev=False):
        """nct_lut_accum_add[_dev]: offer source and result images (any shape [..., 3], uint8 BGR); mask (bytes, one per pixel): only the pixels with mask >= 128"""
        s_, r = np.ascontiguousarray(src, np.uint8).reshape(-1, 3), np.ascontiguousarray(res, np.uint8).reshape(-1, 3)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        assert s_.shape == r.shape and (m is None or len(m) == len(s_))
        with self._seam("lut_accum_add", dev) as s:
            s.call(s.put(s_), s.put(r), s.put(m), len(s_))

    def lut_accum_add_run(self):
        """nct_lut_accum_add_run: offer the images pair_fit_lut would read after the context's last finished run, from where they lie on the device"""
        self._chk(self._l.nct_lut_accum_add_run(self._h))

    def lut_accum_info(self):
        """nct_lut_accum_info -> {"size", "adds", "pixels_offered", "pixels_kept"}"""
        size, rest = C.c_int(), [C.c_uint64() for _ in range(3)]
        self._chk(self._l.nct_lut_accum_info(self._h, C.byref(size), *[C.byref(v) for v in rest]))
        return dict(zip(("size", "adds", "pixels_offered", "pixels_kept"), [size.value] + [v.value for v in rest]))

    def lut_accum_solve(self, lam=None, want_stages=False, *, dev=False):
        """nct_lut_accum_solve[_dev]: the table float32 [N, N, N, 3] over everything added so far (+ {"weight", "resid", "disp"}); lam left out is
        nct_lut_params_default's. The accumulator stays as it is"""
        n = getattr(self, "_lut_accum_size", 1)                    # without an accumulator nothing is written: the library refuses first
        lam = LutParams.default().lambda_ if lam is None else float(lam)
        with self._seam("lut_accum_solve", dev) as s:
            lut, st, cs = self._lut_outputs(s, n, n)
            s.call(lam, lut, C.addressof(cs) if want_stages else None)
            return (s.get(lut), {k: s.get(v) for k, v in st.items()}) if want_stages else s.get(lut)

    def lut_accum_end(self):
        """nct_lut_accum_end: the accumulator's blocks go back"""
        self._chk(self._l.nct_lut_accum_end(self._h))
        self._lut_accum_size = 1

    def pair_fit_lut(self, size=None, lam=None):
        """nct_pair_fit_lut: the table of the context's last finished run, from the images it holds on the device"""
        prm = _lut_params(size, lam)
        N = prm.size if 0 < prm.size <= 65 else 1
        lut = np.empty((N, N, N, 3), np.float32)
        self._chk(self._l.nct_pair_fit_lut(self._h, C.addressof(prm), lut.ctypes.data))
        return lut

    # ---- local colour grids (SPEC §6.22)
    def grid_fit(self, src, res, shape=None, lam=None, want_stages=False, *, dev=False):
        """nct_grid_fit[_dev]: source and result images [h, w, 3] uint8 BGR -> grid float64 [gy, gx, gz, 3, 4] (+ {"sums", "blurred"}, int64 [nodes, 22] each);
        shape = (gy, gx, gz) / lam left out are nct_grid_params_default's"""
        s_, r = np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(res, np.uint8)
        assert s_.ndim == 3 and s_.shape[2] == 3 and s_.shape == r.shape
        prm = _grid_params(shape, lam)
        g = (prm.gy, prm.gx, prm.gz)
        G = _grid_host_shape(*g)
        dg = tuple(max(v, 1) for v in g)                           # the device form reserves what is asked for; the library refuses before it writes
        with self._seam("grid_fit", dev) as s:
            ss, rs = s.put(s_), s.put(r)
            grid = s.new(G + (3, 4), np.float64, dev_shape=dg + (3, 4))
            st = {k: s.new((math.prod(G), 22), np.int64, dev_shape=(math.prod(dg), 22)) for k in ("sums", "blurred")}
            cs = GridStages(st["sums"].ptr, st["blurred"].ptr)
            s.call(ss, rs, s_.shape[0], s_.shape[1], C.addressof(prm), grid, C.addressof(cs) if want_stages else None)
            return (s.get(grid), {k: s.get(v) for k, v in st.items()}) if want_stages else s.get(grid)

    def grid_apply(self, grid, img, *, dev=False, in_place=False):
        """nct_grid_apply[_dev]: grid [gy, gx, gz, 3, 4] float64 on an image [h, w, 3] uint8 BGR of any size -> the image of the same shape. in_place (device
        form): the output over the input"""
        return self._grid_apply("grid_apply", np.uint8, grid, img, dev, in_place)

    def grid_apply_u16(self, grid, img16, *, dev=False, in_place=False):
        """nct_grid_apply_u16[_dev]: grid_apply on an image [h, w, 3] uint16 BGR, a value v standing for the grey level v / 257"""
        return self._grid_apply("grid_apply_u16", np.uint16, grid, img16, dev, in_place)

    def _grid_apply(self, name, dtype, grid, img, dev, in_place):
        """the two applies: the same call on pixels of another depth"""
        t = np.ascontiguousarray(grid, np.float64)
        a = np.ascontiguousarray(img, dtype)
        assert t.ndim == 5 and t.shape[3:] == (3, 4) and a.ndim == 3 and a.shape[2] == 3
        with self._seam(name, dev) as s:
            ts, as_, out = s.put(t), s.put(a), s.new(a.shape, dtype)
            dst = s.over(out, as_ if in_place else None)
            s.call(ts, t.shape[0], t.shape[1], t.shape[2], as_, a.shape[0], a.shape[1], dst)
            return s.get(dst)

    def pair_fit_grid(self, shape=None, lam=None):
        """nct_pair_fit_grid: the grid of the context's last finished run, from the images it holds on the device"""
        prm = _grid_params(shape, lam)
        grid = np.empty(_grid_host_shape(prm.gy, prm.gx, prm.gz) + (3, 4), np.float64)
        self._chk(self._l.nct_pair_fit_grid(self._h, C.addressof(prm), grid.ctypes.data))
        return grid

    def seq_reset(self):
        self._chk(self._l.nct_seq_reset(self._h))

    def seq_end(self):
        self._chk(self._l.nct_seq_end(self._h))
        self._seq = None

    def seq_set_motion(self, radius0=None, radius=None, penalty=None, off=False):
        """nct_seq_set_motion (SPEC §6.4): motion compensation of the open sequence from the next frame on; values left out are nct_seq_motion_default's (3, 1, 1).
        off=True passes NULL; both radii 0 turn it off as well"""
        if off:
            self._chk(self._l.nct_seq_set_motion(self._h, None))
            return
        mp = SeqMotion.default()
        for k, v in (("radius0", radius0), ("radius", radius), ("penalty", penalty)):
            if v is not None:
                setattr(mp, k, int(v))
        self._chk(self._l.nct_seq_set_motion(self._h, C.addressof(mp)))

    def seq_motion_field(self, lab, lab_prev, parent, R, penalty, *, dev=False):
        """nct_seq_motion_field[_dev] (SPEC §6.4 rules 1-3): lab / lab_prev h x w x 3 8-bit Lab, parent None or the coarser level's field int16 [ph, pw, 2] -> int16
        [h, w, 2] of (my, mx)"""
        lab, lp = np.ascontiguousarray(lab, np.uint8), np.ascontiguousarray(lab_prev, np.uint8)
        h, w = lab.shape[:2]
        par = None if parent is None else np.ascontiguousarray(parent, np.int16)
        ph, pw = (0, 0) if par is None else par.shape[:2]
        with self._seam("seq_motion_field", dev) as s:
            ls, lps, pars, out = s.put(lab), s.put(lp), s.put(par), s.new((h, w, 2), np.int16)
            s.call(ls, lps, h, w, pars, ph, pw, int(R), int(penalty), out)
            return s.get(out)

    def seq_blend(self, x, x_prev, lab, lab_prev, tau, sigma, want_tau_map=True, *, dev=False):
        """nct_seq_blend[_dev] (SPEC §6.3 rule 3): x, x_prev [2, h*w, 3] doubles, lab / lab_prev h x w x 3 8-bit Lab -> (X', tau_p map [h, w] or None)"""
        return self._blend("seq_blend", x, x_prev, lab, lab_prev, tau, sigma, None, want_tau_map, False, dev)

    def seq_blend_mc(self, x, x_prev, lab, lab_prev, tau, sigma, field, want_tau_map=True, *, dev=False, alias_prev=False):
        """nct_seq_blend_mc[_dev] (SPEC §6.4 rule 4): seq_blend with L_(t-1) and x_prev read through field (int16 [h, w, 2], or None: seq_blend). alias_prev (device
        form): into x_prev's block, which a field makes an error"""
        return self._blend("seq_blend_mc", x, x_prev, lab, lab_prev, tau, sigma, field, want_tau_map, alias_prev, dev)

    def _blend(self, name, x, x_prev, lab, lab_prev, tau, sigma, field, want_tau_map, alias_prev, dev):
        """the two blends: nct_seq_blend_mc takes the field (or NULL) behind nct_seq_blend's list"""
        lab, lp = np.ascontiguousarray(lab, np.uint8), np.ascontiguousarray(lab_prev, np.uint8)
        h, w = lab.shape[:2]
        a = np.ascontiguousarray(x, np.float64).reshape(-1)
        b = np.ascontiguousarray(x_prev, np.float64).reshape(-1)
        f = None if field is None else np.ascontiguousarray(field, np.int16)
        assert a.size == 6 * h * w and b.size == 6 * h * w and (f is None or f.size == 2 * h * w)
        with self._seam(name, dev) as s:
            ins, fs = [s.put(a), s.put(b), s.put(lab), s.put(lp)], s.put(f)
            out, tm = s.new((2, h * w, 3), np.float64), s.new((h, w), np.float64) if want_tau_map else None
            dst = s.over(out, ins[1] if alias_prev else None)
            s.call(*ins, h, w, tau, sigma, dst, tm, *([fs] if name == "seq_blend_mc" else []))
            return s.get(dst).reshape(2, h * w, 3), s.get(tm)

    def pair_upload(self, src_bgr, ref_bgr):
        s = np.ascontiguousarray(src_bgr, np.uint8)
        r = np.ascontiguousarray(ref_bgr, np.uint8)
        self._pair_shape = s.shape
        self._multi_shapes = [r.shape]
        self._chk(self._l.nct_pair_upload(self._h, s.reshape(-1, 3), s.shape[0], s.shape[1], r.reshape(-1, 3), r.shape[0], r.shape[1]))

    def pair_run(self, params=None, want_timing=False):
        prm = params or Params.default()
        tm = PairTiming() if want_timing else None
        self._chk(self._l.nct_pair_run(self._h, C.addressof(prm), C.addressof(tm) if tm is not None else None))
        return tm.as_dict() if want_timing else None

    def pair_run_levels(self, src_shape, ref_shape, params=None, want_color=False):
        """nct_pair_run_levels on the uploaded pair -> dict of per-level intermediates (lists indexed by level, 0 = coarsest).
        want_color adds "color" (per level the dict of coefficient maps local_color_transfer(want_stages=True) returns) and "labels"."""
        prm = params or Params.default()
        keep, lv, hold = _pair_report(_grids(src_shape, [ref_shape]), prm.levels, want_color)
        return self._run_call("nct_pair_run_levels", prm, keep, lv)

    # ---- source region masks (SPEC §6.11)
    def resize_u8c1(self, img, dh, dw, *, dev=False):
        """nct_resize_u8c1[_dev]: one-channel uint8 image [h, w] -> [dh, dw]"""
        a = np.ascontiguousarray(img, np.uint8)
        with self._seam("resize_u8c1", dev) as s:
            as_, out = s.put(a), s.new((dh, dw), np.uint8)
            s.call(as_, a.shape[0], a.shape[1], out, dh, dw)
            return s.get(out)

    def region_mix(self, x, mask, *, dev=False, in_place=False):
        """nct_region_mix[_dev] (SPEC §6.11 rule 2): x [2, h*w, 3] doubles, mask [h, w] bytes -> X'. in_place (device form): over x"""
        m = np.ascontiguousarray(mask, np.uint8)
        h, w = m.shape
        a = np.ascontiguousarray(x, np.float64).reshape(-1)
        assert a.size == 6 * h * w
        with self._seam("region_mix", dev) as s:
            as_, ms, out = s.put(a), s.put(m), s.new((2, h * w, 3), np.float64)
            dst = s.over(out, as_ if in_place else None)
            s.call(as_, ms, h, w, dst)
            return s.get(dst).reshape(2, h * w, 3)

    def region_compose(self, s_bgr, lab_out, mask, protect=None, params=None, *, dev=False):
        """nct_region_compose[_dev] (SPEC §6.11 rule 3): the source, a finish's 8-bit Lab result and the mask at that size -> the composed BGR image"""
        s_ = np.ascontiguousarray(s_bgr, np.uint8)
        lo, m = np.ascontiguousarray(lab_out, np.uint8), np.ascontiguousarray(mask, np.uint8)
        assert lo.size == s_.size and m.size * 3 == s_.size
        prm, rg = params or Params.default(), _region_params(protect)
        with self._seam("region_compose", dev) as s:
            ss, los, ms, out = s.put(s_), s.put(lo), s.put(m), s.new(s_.shape, np.uint8)
            s.call(ss, los, ms, m.size, C.addressof(rg), C.addressof(prm), out)
            return s.get(out)

    def pair_set_region(self, mask, protect=None):
        """nct_pair_set_region on the uploaded source: mask [h, w] bytes, or None to remove it"""
        if mask is None:
            self._chk(self._l.nct_pair_set_region(self._h, None, None))
            return
        m = _mask_arg(mask, self._pair_shape, "pair_set_region")
        rg = _region_params(protect)
        self._chk(self._l.nct_pair_set_region(self._h, m.ctypes.data, C.addressof(rg)))

    def pair_run_region_levels(self, src_shape, ref_shape, params=None, want_color=True):
        """nct_pair_run_region_levels on the uploaded, masked pair -> pair_run_levels' dict plus per level "mask" [h, w] and "ab_mix" [2, h*w, 3]"""
        prm = params or Params.default()
        g = _grids(src_shape, [ref_shape])
        keep, lv, hold = _pair_report(g, prm.levels, want_color)
        more, rl = _report(RegionLevels, g)
        keep.update(more)
        return self._run_call("nct_pair_run_region_levels", prm, keep, lv, rl)

    def process_pair_region(self, src_bgr, mask, ref_bgr, protect=None, params=None, want_timing=False):
        """nct_process_pair_region: process_pair recolouring only where mask ([h, w] bytes of the source; None: process_pair) says so"""
        m = None if mask is None else _mask_arg(mask, np.shape(src_bgr), "process_pair_region")
        rg = _region_params(protect)
        return self._process("nct_process_pair_region", src_bgr, [m, *self._image(ref_bgr), C.addressof(rg)], params, want_timing)

    def process_pair_fullres_region(self, src_bgr, mask0, ref_bgr, max_side=1000, protect=None, params=None, want_timing=False, finish=0):
        """nct_process_pair_fullres_region (SPEC §6.11 rule 5): mask0 at the source's original size; finish other than FINISH_EXACT goes through
        nct_process_pair_fullres_finish_region (which refuses FINISH_UPSAMPLE with a mask)"""
        m = None if mask0 is None else _mask_arg(mask0, np.shape(src_bgr), "process_pair_fullres_region")
        rg = _region_params(protect)
        if finish == FINISH_EXACT:
            return self._process("nct_process_pair_fullres_region", src_bgr, [m, *self._image(ref_bgr), max_side, C.addressof(rg)], params, want_timing)
        return self._process("nct_process_pair_fullres_finish_region", src_bgr, [m, *self._image(ref_bgr), max_side, int(finish), C.addressof(rg)], params, want_timing)

    def pair_download(self):
        out = np.empty(self._pair_shape, np.uint8)
        self._chk(self._l.nct_pair_download(self._h, out.reshape(-1, 3)))
        return out

    # ---- measurement hooks
    def pm_bench_setup(self, a_chw, b_chw):
        a = np.ascontiguousarray(a_chw, np.float32)
        b = np.ascontiguousarray(b_chw, np.float32)
        Cc, ah, aw = a.shape
        _, bh, bw = b.shape
        self._pm_shape = (ah, aw)
        self._pm_shape_b = (bh, bw)
        self._chk(self._l.nct_pm_bench_setup(self._h, a, b, Cc, ah, aw, bh, bw))

    def pm_bench_run(self, iters=10, rs_max=32, seed=0, count_evals=False, fetch=False):
        ms = C.c_float()
        ev = C.c_uint64()
        ah, aw = self._pm_shape
        nnf = np.empty((ah, aw), np.uint32) if fetch else None
        dist = np.empty((ah, aw), np.float32) if fetch else None
        self._chk(self._l.nct_pm_bench_run(self._h, iters, rs_max, seed, C.byref(ms), C.byref(ev) if count_evals else None,
                                           _ptr(nnf), _ptr(dist)))
        return ms.value, (ev.value if count_evals else None), nnf, dist

    def pm_bench_run_bidir(self, iters=10, rs_max=32, seed=0, pm_mode=1, count=False, fetch=False, both=False):
        """The pipeline's form of the pass (both directions per launch; pm_mode 0 fp32 / 1 fp32 + row rejection / 2 fp16).
        -> (kernel ms, [evals, accepted] or None, ann, annd[, bnn, bnnd])."""
        ms = C.c_float()
        cnt = (C.c_uint64 * 2)()
        ah, aw = self._pm_shape
        bh, bw = self._pm_shape_b
        ann = np.empty((ah, aw), np.uint32) if fetch else None
        annd = np.empty((ah, aw), np.float32) if fetch else None
        bnn = np.empty((bh, bw), np.uint32) if fetch and both else None
        bnnd = np.empty((bh, bw), np.float32) if fetch and both else None
        self._chk(self._l.nct_pm_bench_run_bidir(self._h, iters, rs_max, seed, pm_mode, C.byref(ms), C.addressof(cnt) if count else None,
                                                 _ptr(ann), _ptr(annd), _ptr(bnn), _ptr(bnnd)))
        r = (ms.value, (list(cnt) if count else None), ann, annd)
        return r + (bnn, bnnd) if both else r


# the seams whose device form also has a method of its own, X_dev(...) = X(..., dev=True); a new seam gets one body and, only if it needs this spelling, a row here
_DEV_SPELLING = ("color_finish_upsample", "color_finish_guided", "color_finish_upsample_region", "color_finish_guided_region", "select_reference", "region_pull", "seq_warp",
                 "seq_blend", "seq_blend_mc", "seq_motion_field", "seq_change", "lut_fit", "lut_fit_masked", "lut_apply", "resize_u8c1", "region_mix", "region_compose")
for _name in _DEV_SPELLING:
    setattr(Context, _name + "_dev", functools.partialmethod(getattr(Context, _name), dev=True))
