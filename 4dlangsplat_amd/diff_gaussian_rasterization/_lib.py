"""ctypes binding of liblsr.so (include/lsr.h).  No torch types cross the boundary: only device
pointers, sizes and the HIP stream handle.  Boundary (below) is the one place a tensor becomes such a
pointer: no other module of the package calls .data_ptr() for an argument or a struct field.

The library is built in-tree (4dlangsplat_amd/csrc/Makefile -> 4dlangsplat_amd/build/liblsr.so).
There is no fallback: if the library is missing, importing the rasterizer raises.
"""
from __future__ import annotations

import ctypes
import os

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("LSR_LIBRARY", os.path.join(_PKG, "build", "liblsr.so"))

c_float_p = ctypes.c_void_p  # device pointers are passed as opaque addresses
API_VERSION = 4               # LSR_API_VERSION of the include/lsr.h these structs mirror
DEFORM_API_VERSION = 3        # LSR_DEFORM_API_VERSION of include/lsr_deform.h (DeformNet, DeformGrads)
QUERY_API_VERSION = 1         # LSR_QUERY_API_VERSION of include/lsr_query.h (Decoder)
VIDEO_API_VERSION = 1         # LSR_VIDEO_API_VERSION of include/lsr_video.h
AE_API_VERSION = 1            # LSR_AE_API_VERSION of include/lsr_autoencoder.h (AeParams, Autoencoder)


class Settings(ctypes.Structure):
    _fields_ = [
        ("image_height", ctypes.c_int32), ("image_width", ctypes.c_int32),
        ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float),
        ("bg", ctypes.c_void_p), ("scale_modifier", ctypes.c_float),
        ("viewmatrix", ctypes.c_void_p), ("projmatrix", ctypes.c_void_p),
        ("sh_degree", ctypes.c_int32), ("campos", ctypes.c_void_p),
        ("prefiltered", ctypes.c_int32), ("debug", ctypes.c_int32), ("include_feature", ctypes.c_int32),
    ]


class FwdIn(ctypes.Structure):
    _fields_ = [
        ("P", ctypes.c_int32), ("M", ctypes.c_int32), ("C", ctypes.c_int32),
        ("means3D", ctypes.c_void_p), ("shs", ctypes.c_void_p), ("colors_precomp", ctypes.c_void_p),
        ("language_feature", ctypes.c_void_p), ("opacities", ctypes.c_void_p), ("scales", ctypes.c_void_p),
        ("rotations", ctypes.c_void_p), ("cov3D_precomp", ctypes.c_void_p),
        ("language_feature_split", ctypes.c_void_p),
    ]


class FwdOut(ctypes.Structure):
    _fields_ = [("out_color", ctypes.c_void_p), ("out_language_feature", ctypes.c_void_p),
                ("radii", ctypes.c_void_p), ("out_depth", ctypes.c_void_p)]


class BwdIn(ctypes.Structure):
    _fields_ = [("dL_dout_color", ctypes.c_void_p), ("dL_dout_language_feature", ctypes.c_void_p),
                ("dL_dout_depth", ctypes.c_void_p), ("deterministic", ctypes.c_int32)]


class BwdOut(ctypes.Structure):
    _fields_ = [("dL_dmeans3D", ctypes.c_void_p), ("dL_dmeans2D", ctypes.c_void_p), ("dL_dcolors", ctypes.c_void_p),
                ("dL_dlanguage_feature", ctypes.c_void_p), ("dL_dopacity", ctypes.c_void_p),
                ("dL_dcov3D", ctypes.c_void_p), ("dL_dsh", ctypes.c_void_p), ("dL_dscales", ctypes.c_void_p),
                ("dL_drotations", ctypes.c_void_p)]


# every symbol include/lsr.h declares, with its ctypes signature
class DeformNet(ctypes.Structure):
    """include/lsr_deform.h lsr_deform_net (LSR_DEFORM_API_VERSION 3)"""
    _fields_ = [("n_scales", ctypes.c_int32), ("channels", ctypes.c_int32), ("width", ctypes.c_int32),
                ("res", ctypes.c_int32 * 4), ("multires", ctypes.c_int32 * 4), ("depth", ctypes.c_int32),
                ("heads", ctypes.c_uint32), ("apply_rotation", ctypes.c_int32), ("lang_mode", ctypes.c_int32),
                ("lang_dim", ctypes.c_int32), ("centers", ctypes.c_int32), ("time_pe", ctypes.c_int32),
                ("aabb", ctypes.c_void_p), ("planes", (ctypes.c_void_p * 6) * 4),
                ("w_feat", ctypes.c_void_p * 4), ("b_feat", ctypes.c_void_p * 4),
                ("w1", ctypes.c_void_p * 6), ("b1", ctypes.c_void_p * 6), ("w2", ctypes.c_void_p * 6),
                ("b2", ctypes.c_void_p * 6), ("w_lang", ctypes.c_void_p * 3), ("b_lang", ctypes.c_void_p * 3)]


class DeformGrads(ctypes.Structure):
    """include/lsr_deform.h lsr_deform_grads"""
    _fields_ = [("planes", (ctypes.c_void_p * 6) * 4), ("w_feat", ctypes.c_void_p * 4), ("b_feat", ctypes.c_void_p * 4),
                ("w1", ctypes.c_void_p * 6), ("b1", ctypes.c_void_p * 6), ("w2", ctypes.c_void_p * 6),
                ("b2", ctypes.c_void_p * 6), ("w_lang", ctypes.c_void_p * 3), ("b_lang", ctypes.c_void_p * 3),
                ("aabb", ctypes.c_void_p)]


class AdamGroup(ctypes.Structure):
    """include/lsr_train.h lsr_adam_group"""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int64), ("lr", ctypes.c_double),
                ("step", ctypes.c_int64)]


class RowTensor(ctypes.Structure):
    """include/lsr_train.h lsr_row_tensor"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("row_bytes", ctypes.c_int64),
                ("zero_from", ctypes.c_int64)]


class SegView(ctypes.Structure):
    """include/lsr_train.h lsr_seg_view"""
    _fields_ = [("image", ctypes.c_void_p), ("d_image", ctypes.c_void_p), ("seg", ctypes.c_void_p),
                ("table", ctypes.c_void_p), ("n_seg", ctypes.c_int32)]


class Decoder(ctypes.Structure):
    """include/lsr_query.h lsr_decoder"""
    _fields_ = [("n_layers", ctypes.c_int32), ("dims", ctypes.c_int32 * 9), ("weight", ctypes.c_void_p * 8),
                ("bias", ctypes.c_void_p * 8)]


class AeParams(ctypes.Structure):
    """include/lsr_autoencoder.h lsr_ae_params"""
    _fields_ = [(n, ctypes.c_void_p * 8) for n in ("enc_w", "enc_b", "bn_w", "bn_b", "dec_w", "dec_b")]


class Autoencoder(ctypes.Structure):
    """include/lsr_autoencoder.h lsr_autoencoder"""
    _fields_ = [("n_enc", ctypes.c_int32), ("n_dec", ctypes.c_int32), ("feature_dim", ctypes.c_int32),
                ("enc_dims", ctypes.c_int32 * 8), ("dec_dims", ctypes.c_int32 * 8), ("p", AeParams),
                ("bn_mean", ctypes.c_void_p * 8), ("bn_var", ctypes.c_void_p * 8), ("bn_count", ctypes.c_void_p * 8)]


class PlaneDesc(ctypes.Structure):
    """include/lsr_plane_reg.h lsr_plane_desc"""
    _fields_ = [("t", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("C", ctypes.c_int32), ("H", ctypes.c_int32),
                ("W", ctypes.c_int32), ("w_smooth", ctypes.c_double), ("w_l1", ctypes.c_double)]


ADAM_MAX_GROUPS = 16        # LSR_ADAM_MAX_GROUPS
GATHER_MAX_TENSORS = 32     # LSR_GATHER_MAX_TENSORS
SEG_LOSS_MAX_VIEWS = 8      # lsr_seg_loss_views' V
QUERY_MAX_LAYERS = 8        # LSR_QUERY_MAX_LAYERS
QUERY_MAX_PHRASES = 64      # LSR_QUERY_MAX_PHRASES
QUERY_MAX_WIDTH = 512       # LSR_QUERY_MAX_WIDTH
QUERY_MAX_INPUT = 32        # LSR_QUERY_MAX_INPUT
SEGMENT_MAX_SCALE = 63      # LSR_SEGMENT_MAX_SCALE (include/lsr_segment.h)
SEGMENT_MAX_SIDE = 16384    # LSR_SEGMENT_MAX_SIDE
SEGMENT_STRATEGIES = {"point": 0, "mean": 1}   # LSR_SEGMENT_POINT, LSR_SEGMENT_MEAN
PCA_MIN_CHANNELS = 4        # LSR_PCA_MIN_CHANNELS (include/lsr_pca.h)
PCA_MAX_CHANNELS = 32       # LSR_PCA_MAX_CHANNELS
PCA_BLOCK_PIXELS = 2048     # LSR_PCA_BLOCK_PIXELS
PCA_TILE_PIXELS = 256       # LSR_PCA_TILE_PIXELS
PCA_FINISH_WAVES = 16       # LSR_PCA_FINISH_WAVES
PCA_RANGE_THREADS = 256     # LSR_PCA_RANGE_THREADS
CENTERS_MAX_K = 8           # LSR_CENTERS_MAX_K (include/lsr_centers.h)
CENTERS_MAX_SAMPLES = 256   # LSR_CENTERS_MAX_SAMPLES
CENTERS_MAX_DIM = 32        # LSR_CENTERS_MAX_DIM
PLANE_REG_API_VERSION = 1   # LSR_PLANE_REG_API_VERSION (include/lsr_plane_reg.h)
PLANE_REG_MAX_PLANES = 24   # LSR_PLANE_REG_MAX_PLANES
PLANE_REG_BLOCK_ELEMS = 1024  # LSR_PLANE_REG_BLOCK_ELEMS
VIDEO_MAX_WIDTH = 4096      # LSR_VIDEO_MAX_WIDTH (include/lsr_video.h)
VIDEO_MAX_QUERIES = 16      # LSR_VIDEO_MAX_QUERIES
VIDEO_ROW_TILE = 128        # LSR_VIDEO_ROW_TILE
VIDEO_COL_TILE = 128        # LSR_VIDEO_COL_TILE
AE_MAX_LAYERS = 8           # LSR_AE_MAX_LAYERS (include/lsr_autoencoder.h)
AE_MAX_WIDTH = 4096         # LSR_AE_MAX_WIDTH
AE_MAX_LATENT = 32          # LSR_AE_MAX_LATENT
AE_MAX_BATCH = 64           # LSR_AE_MAX_BATCH
AE_EVAL_CHUNK = 2048        # LSR_AE_EVAL_CHUNK
TILES_LEVELS = 4            # LSR_TILES_LEVELS (include/lsr_tiles.h)
TILES_MAX_LABEL = 1023      # LSR_TILES_MAX_LABEL
TILES_MAX_TILES = 4 * 1023  # LSR_TILES_MAX_TILES
TILES_SIDE = 224            # LSR_TILES_SIDE
TILES_MAX_SIDE = 16384      # LSR_TILES_MAX_SIDE
TILES_DESC_INTS = 6         # LSR_TILES_DESC_INTS
TILES_COUNTS = 5            # LSR_TILES_COUNTS

_vp = ctypes.c_void_p
SIGNATURES = {
    "lsr_adam_step": (ctypes.c_int, [ctypes.POINTER(AdamGroup), ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_double, _vp]),
    "lsr_densify_stats": (ctypes.c_int, [ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsr_train_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32]),
    "lsr_densify_plan": (ctypes.c_int, [ctypes.c_int32, _vp, _vp, _vp, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsr_prune_plan": (ctypes.c_int, [ctypes.c_int32, _vp, _vp, _vp, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                      _vp, _vp, _vp, _vp]),
    "lsr_gather_rows": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(RowTensor), _vp, ctypes.c_int64, _vp]),
    "lsr_split_fixup": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
    "lsr_reset_opacity": (ctypes.c_int, [ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsr_activate": (ctypes.c_int, [ctypes.c_int32] + [_vp] * 7),
    "lsr_l1_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32]),
    "lsr_l1_loss_views": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp, _vp]),
    "lsr_l1_loss_views_backward": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp,
                                                  _vp]),
    "lsr_image_loss_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 4),
    "lsr_image_loss_views": (ctypes.c_int, [ctypes.c_int32] * 4 + [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lsr_image_loss_views_backward": (ctypes.c_int, [ctypes.c_int32] * 4 + [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp,
                                                                             _vp, _vp]),
    "lsr_seg_loss_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 4),
    "lsr_seg_loss_views": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.POINTER(SegView), ctypes.c_float,
                                          ctypes.c_float, ctypes.c_int32, _vp, _vp, _vp]),
    "lsr_seg_loss_views_backward": (ctypes.c_int, [ctypes.c_int32] * 4 + [ctypes.POINTER(SegView), ctypes.c_float,
                                                   ctypes.c_float, ctypes.c_int32, _vp, _vp, _vp]),
    "lsr_repeat_rows": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(RowTensor), ctypes.c_int64, ctypes.c_int32, _vp]),
    "lsr_sum_row_blocks": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(RowTensor), ctypes.c_int64, ctypes.c_int32,
                                          _vp]),
    "lsr_activate_backward": (ctypes.c_int, [ctypes.c_int32] + [_vp] * 10),
    "lsr_version": (ctypes.c_int, []),
    "lsr_require_api": (ctypes.c_int, [ctypes.c_int32]),
    "lsr_deform_require_api": (ctypes.c_int, [ctypes.c_int32]),
    "lsr_last_error": (ctypes.c_char_p, []),
    "lsr_geom_bytes": (ctypes.c_int64, [ctypes.c_int32]),
    "lsr_binning_bytes": (ctypes.c_int64, [ctypes.c_int64]),
    "lsr_img_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "lsr_backward_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "lsr_forward_preprocess": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn), ctypes.POINTER(FwdOut),
                                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "lsr_forward_preprocess_async": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn),
                                                    ctypes.POINTER(FwdOut), ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p]),
    "lsr_forward_preprocess_views_async": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                          ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.POINTER(FwdOut)),
                                                          ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                                          ctypes.c_void_p]),
    "lsr_forward_preprocess_views_split_async": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32,
                                                                ctypes.POINTER(ctypes.POINTER(Settings)),
                                                                ctypes.POINTER(FwdIn),
                                                                ctypes.POINTER(ctypes.POINTER(FwdOut)),
                                                                ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                                                ctypes.c_void_p]),
    "lsr_forward_preprocess_views_rows_async": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                               ctypes.POINTER(ctypes.POINTER(Settings)),
                                                               ctypes.POINTER(FwdIn),
                                                               ctypes.POINTER(ctypes.POINTER(FwdOut)),
                                                               ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]),
    "lsr_forward_depth_order_views_async": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                           ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.c_void_p),
                                                           ctypes.c_void_p, ctypes.c_void_p]),
    "lsr_forward_binning_views": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                 ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "lsr_binning_bytes_tb": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]),
    "lsr_forward_preprocess_views_tb_async": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                             ctypes.POINTER(ctypes.POINTER(Settings)),
                                                             ctypes.POINTER(FwdIn),
                                                             ctypes.POINTER(ctypes.POINTER(FwdOut)),
                                                             ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]),
    "lsr_forward_instance_scan_views_async": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                             ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.c_void_p),
                                                             ctypes.c_void_p, ctypes.c_void_p]),
    "lsr_forward_binning_views_tb": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                    ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.c_void_p),
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                    ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "lsr_forward_render": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn), ctypes.POINTER(FwdOut),
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_void_p]),
    "lsr_forward_binning": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn), ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "lsr_forward_composite": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn), ctypes.POINTER(FwdOut),
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_void_p]),
    "lsr_forward_composite_views": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                   ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.POINTER(FwdOut)),
                                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                   ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64),
                                                   ctypes.c_void_p]),
    "lsr_backward_composite_views": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                    ctypes.POINTER(FwdIn), ctypes.POINTER(ctypes.POINTER(BwdIn)),
                                                    ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                    ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "lsr_backward": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn), ctypes.POINTER(BwdIn),
                                    ctypes.POINTER(BwdOut), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]),
    "lsr_backward_views": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)), ctypes.POINTER(FwdIn),
                                          ctypes.POINTER(ctypes.POINTER(BwdIn)), ctypes.POINTER(BwdOut),
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64),
                                          ctypes.c_int32, ctypes.c_void_p]),
    "lsr_backward_composite": (ctypes.c_int, [ctypes.POINTER(Settings), ctypes.POINTER(FwdIn), ctypes.POINTER(BwdIn),
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_int64, ctypes.c_void_p]),
    "lsr_backward_preprocess_views": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                     ctypes.POINTER(FwdIn), ctypes.POINTER(BwdOut),
                                                     ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, ctypes.c_void_p]),
    "lsr_backward_preprocess_views_rows": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.POINTER(Settings)),
                                                          ctypes.POINTER(FwdIn), ctypes.POINTER(BwdOut),
                                                          ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32,
                                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "lsr_language_split": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "lsr_radii_max": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p,
                                     ctypes.c_int32, ctypes.c_void_p]),
    "lsr_mark_visible": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "lsr_profile_enable": (ctypes.c_int, [ctypes.c_int32]),
    "lsr_profile_phases": (ctypes.c_int, [ctypes.c_uint32]),
    "lsr_knn_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32]),
    "lsr_knn_mean_dist": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p]),
    "lsr_deform_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(DeformNet)]),
    "lsr_deform_prepare": (ctypes.c_int, [ctypes.POINTER(DeformNet), ctypes.c_void_p, ctypes.c_void_p]),
    "lsr_deform_forward": (ctypes.c_int, [ctypes.POINTER(DeformNet), ctypes.c_void_p, ctypes.c_int32]
                           + [ctypes.c_void_p] * 14 + [ctypes.c_void_p]),
    "lsr_deform_backward_scratch_bytes": (ctypes.c_int64, [ctypes.POINTER(DeformNet), ctypes.c_int32]),
    "lsr_deform_backward": (ctypes.c_int, [ctypes.POINTER(DeformNet), ctypes.c_void_p, ctypes.c_int32]
                            + [ctypes.c_void_p] * 14 + [ctypes.POINTER(DeformGrads), ctypes.c_void_p, ctypes.c_void_p]),
    "lsr_query_require_api": (ctypes.c_int, [ctypes.c_int32]),
    "lsr_query_relevancy": (ctypes.c_int, [ctypes.POINTER(Decoder), ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int32, _vp, ctypes.c_int32, _vp, ctypes.c_float, _vp, _vp]),
    "lsr_query_decode": (ctypes.c_int, [ctypes.POINTER(Decoder), ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int64,
                                        _vp, _vp]),
    "lsr_segment_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32] * 3),
    "lsr_segment": (ctypes.c_int, [ctypes.c_int32] * 3 + [_vp, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, _vp,
                                   ctypes.c_int32] + [_vp] * 8),
    "lsr_pca_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64]),
    "lsr_pca_sums": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                    _vp, _vp, _vp]),
    "lsr_pca_gram": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int64, _vp,
                                    ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp]),
    "lsr_pca_basis": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64] + [_vp] * 6),
    "lsr_pca_project": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp,
                                       ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsr_pca_colorize_f32": (ctypes.c_int, [ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lsr_pca_colorize_u8": (ctypes.c_int, [ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lsr_centers_kmeans": (ctypes.c_int, [_vp] + [ctypes.c_int32] * 5 + [_vp] * 5),
    "lsr_centers_from_field": (ctypes.c_int, [ctypes.POINTER(DeformNet), _vp, ctypes.c_int32, _vp, _vp, ctypes.c_uint32]
                               + [ctypes.c_int32] * 3 + [_vp] * 7),
    "lsr_plane_reg_workspace_bytes": (ctypes.c_int64, [ctypes.c_int32, ctypes.POINTER(PlaneDesc)]),
    "lsr_plane_reg": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(PlaneDesc), ctypes.c_int32] + [_vp] * 5),
    "lsr_video_require_api": (ctypes.c_int, [ctypes.c_int32]),
    "lsr_video_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(Decoder), ctypes.c_int64]),
    "lsr_video_cosine": (ctypes.c_int, [ctypes.POINTER(Decoder), ctypes.c_int64, _vp, ctypes.c_int32, _vp, _vp, _vp,
                                        ctypes.c_int64, _vp]),
    "lsr_video_segment_mean": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    "lsr_ae_require_api": (ctypes.c_int, [ctypes.c_int32]),
    "lsr_ae_workspace_size": (ctypes.c_int64, [ctypes.POINTER(Autoencoder), ctypes.c_int64, ctypes.c_int32]),
    "lsr_ae_encode": (ctypes.c_int, [ctypes.POINTER(Autoencoder), ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, _vp]),
    "lsr_ae_eval_loss": (ctypes.c_int, [ctypes.POINTER(Autoencoder), ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64,
                                        _vp]),
    "lsr_ae_train_step": (ctypes.c_int, [ctypes.POINTER(Autoencoder), ctypes.POINTER(AeParams),
                                         ctypes.POINTER(AeParams), ctypes.c_int32, _vp] + [ctypes.c_double] * 4
                          + [ctypes.c_int64, ctypes.c_double, _vp, _vp, ctypes.c_int64, _vp]),
    "lsr_tiles_workspace_size": (ctypes.c_int64, [ctypes.c_int32]),
    "lsr_tiles_census": (ctypes.c_int, [ctypes.c_int32] * 3 + [_vp, ctypes.c_int64, _vp, _vp]),
    "lsr_tiles_plan": (ctypes.c_int, [ctypes.c_int32] * 3 + [ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lsr_tiles_render": (ctypes.c_int, [ctypes.c_int32] * 3 + [_vp, _vp, ctypes.c_int64, _vp, _vp,
                                                               ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, _vp, _vp,
                                                               _vp]),
    "lsr_profile_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64),
                                        ctypes.c_int32]),
}

PHASES = ["preprocess", "depth_sort", "instance_scan", "emit", "tile_sort", "tile_ranges", "render_fwd",
          "render_bwd", "preprocess_bwd", "preprocess_bwd_views"]


def profile_enable(on=True, phases=None):
    """Start (resetting the totals) or stop event timing; `phases` limits it to those names."""
    L = load()
    L.lsr_profile_phases(0xFFFFFFFF if phases is None else sum(1 << PHASES.index(p) for p in phases))
    L.lsr_profile_enable(1 if on else 0)


def profile_read():
    """{phase: (total_ms, launches)} of the event-timed phases since profile_enable()."""
    n = len(PHASES)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    load().lsr_profile_read(ms, cnt, n)
    return {PHASES[i]: (ms[i], cnt[i]) for i in range(n)}

_LIB = None


def load():
    """Load liblsr.so (raises if it has not been built)."""
    global _LIB
    if _LIB is None:
        path = os.environ.get("LSR_LIBRARY", LIB_PATH)   # variant builds for profiling experiments
        if not os.path.exists(path):
            raise ImportError(f"liblsr.so not found at {LIB_PATH}; build it with `make -C 4dlangsplat_amd/csrc` "
                              "(or __graft_entry__.build()).  There is no CPU fallback.")
        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if (lib.lsr_require_api(API_VERSION) != 0 or lib.lsr_deform_require_api(DEFORM_API_VERSION) != 0
                or lib.lsr_query_require_api(QUERY_API_VERSION) != 0
                or lib.lsr_video_require_api(VIDEO_API_VERSION) != 0
                or lib.lsr_ae_require_api(AE_API_VERSION) != 0):
            raise ImportError(f"{path}: {lib.lsr_last_error().decode()} (rebuild it: make -C 4dlangsplat_amd/csrc)")
        _LIB = lib
    return _LIB


class Boundary:
    """What may cross into liblsr.so for a call that runs on `device`: the address of a contiguous tensor of
    the dtype the C side reads, on that device, and a stream of that device.  Anything else raises ValueError
    before an address is taken; ok() is the same test as a bool, for the callers that fall back to torch.
    Nothing is converted, copied or allocated here, and no device guard is entered.  ptr / opt / array return bare
    integers that keep nothing alive: the caller holds the tensor until the call is enqueued, so a copy made for the
    call (.contiguous(), .to()) is bound to a name first, never written inside the boundary's argument."""
    __slots__ = ("device",)

    def __init__(self, device):
        if not isinstance(device, torch.device):
            device = torch.device(device)
        if device.type == "cuda" and device.index is None:   # "cuda": the current device, as torch places tensors
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device    # with its index, as tensor.device gives it

    def ok(self, t, dtype=torch.float32, strided=False) -> bool:
        return (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device
                and (strided or t.is_contiguous()))

    def ptr(self, t, name="tensor", dtype=torch.float32, strided=False) -> int:
        """The address of `t`.  strided=True is for the entry points that take the tensor's strides as arguments of
        their own: the caller passes them, so `t` need not be contiguous."""
        if not self.ok(t, dtype, strided):
            raise ValueError(f"{name}: {'' if strided else 'contiguous '}{_short(dtype)} tensor on {self.device} "
                             f"required, got {_found(t)}")
        return t.data_ptr()

    def opt(self, t, name="tensor", dtype=torch.float32):
        """ptr(), or None (NULL) for None"""
        return None if t is None else self.ptr(t, name, dtype)

    def array(self, tensors, name="tensors", dtype=torch.float32):
        """(c_void_p * n) over the addresses of `tensors`, each checked as `name[i]`"""
        for i, t in enumerate(tensors):
            if not self.ok(t, dtype):
                self.ptr(t, f"{name}[{i}]", dtype)   # raises, naming the element
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def stream(self, stream=None):
        """the native calls' stream argument: `stream` (a torch stream of this device) or the device's current one"""
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        elif stream.device != self.device:
            raise ValueError(f"stream: a stream of {self.device} required, got one of {stream.device}")
        return ctypes.c_void_p(stream.cuda_stream)


HOST = Boundary(torch.device("cpu"))   # for the pinned host buffers a native call writes its counts to


def _short(dtype):
    return str(dtype).replace("torch.", "")


def _found(t):
    if not isinstance(t, torch.Tensor):
        return type(t).__name__
    return f"{'' if t.is_contiguous() else 'non-contiguous '}{_short(t.dtype)} on {t.device}"


def check(rc: int, what: str):
    if rc != 0:
        msg = load().lsr_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
