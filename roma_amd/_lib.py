"""ctypes binding of libroma_hip.so (include/roma_hip.h).  Loading never falls back: a missing library is an error."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_long, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libroma_hip.so")

ROMA_F32, ROMA_F16, ROMA_BF16 = 0, 1, 2
ROMA_NCHW, ROMA_NHWC = 0, 1
LC_VARIANTS = {"auto": 0, "tile8x4": 1, "tile8x8": 2, "rows8": 3}
ABI_VERSION = 5
SCORE_MSAC, SCORE_MAGSAC = 0, 1                            # the `scoring` argument of the roma_*_ex estimator calls
ROMA_E_ARG, ROMA_E_DTYPE, ROMA_E_SHAPE, ROMA_E_ALIGN, ROMA_E_UNSUPPORTED = -1, -2, -3, -4, -5      # include/roma_hip.h

# name -> argtypes; restype is c_int unless listed in _RESTYPES.  Mirrors include/roma_hip.h one to one.
SIGNATURES = {
    "roma_abi_version": [],
    "roma_last_error": [],
    "roma_local_corr": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                        c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_warp_bilinear": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                           c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_disp_emb": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_void_p],
    "roma_interp_bilinear": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_interp_bilinear_pair": [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_refiner_assemble": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_int, c_int, c_float, c_int, c_void_p],
    "roma_project_skinny": [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_flow_update": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p],
    "roma_cls_to_flow_refine": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_long, c_long, c_int, c_void_p],
    "roma_cos_kernel": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                        c_float, c_void_p],
    "roma_add_layernorm": [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_long,
                           c_long, c_int, c_float, c_void_p],
    "roma_attention_fwd": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int] + [c_long] * 12 + [c_float, c_int, c_void_p],
    "roma_chol_diag_block": [c_void_p, c_int, c_long, c_void_p, c_int, c_long, c_int, c_int, c_void_p, c_int, c_void_p],
    "roma_chol_step": [c_void_p, c_int, c_long, c_int, c_int, c_int, c_int, c_void_p, c_int, c_long, c_void_p, c_int, c_long,
                       c_void_p, c_int, c_long, c_void_p, c_int, c_int, c_void_p],
    "roma_chol_subst_step": [c_int, c_void_p, c_int, c_long, c_void_p, c_long, c_long, c_int, c_void_p, c_long, c_long, c_int, c_int,
                             c_void_p, c_int, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_match_finalize": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_kde_density": [c_void_p, c_void_p, c_int, c_int, c_float, c_int, c_void_p],
    "roma_nn_argmin": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "roma_race_keys": [c_void_p, c_void_p, c_void_p, c_long, c_float, ctypes.c_uint, ctypes.c_uint, c_void_p],
    "roma_race_select_workspace": [c_int, c_long, c_int],
    "roma_race_select": [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_float, ctypes.c_uint, c_void_p, c_void_p, c_void_p, c_long,
                         c_void_p],
    "roma_kde_density_batch": [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_float, c_int, c_void_p],
    "roma_dwconv5x5_bn_relu": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_resample_u8": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p],
    "roma_normalize_u8": [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p],
    "roma_bias_relu_nchw": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "roma_bias_relu_pool2_nchw": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_bias_relu_nhwc": [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p],
    "roma_bias_relu_pool2_nhwc": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_maxpool2_nhwc": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_conv3x3_bias_relu": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_conv3x3_bias_relu_instances": [c_int, c_char_p, c_int],
    "roma_pointwise_mfma": [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_refiner_block": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                           c_int, c_int, c_void_p],
    "roma_refiner_block_mid": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_void_p],
    "roma_refiner_wide_pack": [c_void_p, c_void_p, c_int],
    "roma_refiner_wide_taps": [c_void_p, c_void_p, c_int],
    "roma_jpeg_info": [c_void_p, c_long, c_void_p],
    "roma_jpeg_entropy_decode": [c_void_p, c_long, c_void_p, c_void_p],
    "roma_jpeg_reconstruct": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_refiner_block_wide": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                c_int, c_void_p],
    "roma_refiner_head": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                          c_float, c_float, c_void_p],
    "roma_pointwise_small": [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p],
    "roma_tiny_corr_posembed": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "roma_ransac_workspace": [c_int, c_int, c_int, c_int, c_void_p],
    "roma_ransac_hypotheses": [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, ctypes.c_uint, c_int, c_void_p, c_long, c_void_p],
    "roma_ransac_select": [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_long, c_void_p, c_void_p,
                           c_void_p],
    "roma_ransac_hypotheses_ex": [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, ctypes.c_uint, c_int, c_void_p, c_long,
                                  c_void_p],
    "roma_ransac_select_ex": [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_long, c_void_p, c_void_p,
                              c_void_p],
    "roma_magsac_table": [c_void_p, c_void_p],
    "roma_essential_workspace": [c_int, c_int, c_int, c_void_p],
    "roma_essential_hypotheses": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, ctypes.c_uint, c_int, c_void_p,
                                  c_long, c_void_p],
    "roma_essential_select": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_long, c_void_p,
                              c_void_p, c_void_p],
    "roma_essential_hypotheses_ex": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, ctypes.c_uint, c_int,
                                     c_void_p, c_long, c_void_p],
    "roma_essential_select_ex": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_long,
                                 c_void_p, c_void_p, c_void_p],
    "roma_recover_pose": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_void_p],
    "roma_refine_pose": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int,
                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_refine_fundamental": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p],
    "roma_refine_homography": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p],
    "roma_triangulate": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float,
                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_triangulate_nview": [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_long,
                               c_float, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p],
    "roma_tracks_workspace": [c_int, c_void_p, c_int, c_void_p],
    "roma_build_tracks": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "roma_warp_kpts": [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                       ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_dense_match_metrics": [c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                 c_int, c_int, ctypes.c_double, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_absolute_pose_workspace": [c_int, c_int, c_int, c_void_p],
    "roma_absolute_pose_hypotheses": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, ctypes.c_uint, c_int, c_void_p,
                                      c_long, c_void_p],
    "roma_absolute_pose_select": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p, c_long, c_void_p,
                                  c_void_p, c_void_p, c_void_p],
    "roma_refine_absolute_pose": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_similarity_workspace": [c_int, c_int, c_int, c_void_p],
    "roma_similarity_hypotheses": [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int, ctypes.c_uint, c_int, c_void_p, c_long,
                                   c_void_p],
    "roma_similarity_select": [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_refine_similarity": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    "roma_bundle_workspace": [c_int, c_int, c_void_p],
    "roma_bundle_adjust": [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_uint,
                           ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_long, c_void_p],
    "roma_rotation_average": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p],
    "roma_positions_workspace": [c_int, c_int, c_int, c_void_p],
    "roma_global_positions": [c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                              ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                              c_void_p],
    "roma_depth_fuse_workspace": [c_int, c_long, c_void_p],
    "roma_depth_fuse": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, ctypes.c_double, ctypes.c_double, c_int, c_int, c_void_p,
                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "roma_render_points_workspace": [c_int, c_int, c_int, c_void_p],
    "roma_render_points": [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_double, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p],
}
_RESTYPES = {"roma_last_error": c_char_p, "roma_ransac_workspace": c_long, "roma_essential_workspace": c_long,
             "roma_race_select_workspace": c_long, "roma_absolute_pose_workspace": c_long, "roma_similarity_workspace": c_long,
             "roma_tracks_workspace": c_long, "roma_bundle_workspace": c_long, "roma_depth_fuse_workspace": c_long,
             "roma_positions_workspace": c_long, "roma_render_points_workspace": c_long}

_lib = None


class RomaHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libroma_hip.so (once).  Raises if it has not been built — there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RomaHipError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"or `make -C roma_amd/csrc`.  roma_amd has no CPU/PyTorch fallback for its kernels.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
    if lib.roma_abi_version() != ABI_VERSION:
        raise RomaHipError(f"libroma_hip.so ABI {lib.roma_abi_version()} != binding ABI {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc == 0:
        return
    msg = load().roma_last_error().decode(errors="replace")
    if rc < 0:
        raise ValueError(f"{what}: {msg} (code {rc})")
    raise RomaHipError(f"{what}: HIP error {rc}: {msg}")
