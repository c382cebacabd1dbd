"""ctypes binding of libobjnerf_hip.so (include/objnerf_hip.h).

The library is built in-tree (openobj_amd/csrc/libobjnerf_hip.so, `make -C openobj_amd/csrc` or
`__graft_entry__.build()`).  There is NO fallback: if it is missing, or a call returns an error
code, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

# torch must be imported BEFORE libobjnerf_hip.so is dlopen'ed: the torch wheel bundles its own
# libamdhip64.so.7 and both must share ONE HIP runtime in the process (streams, device pointers).
# Loading ours first would bind /opt/rocm's runtime and kernel launches on torch's streams fail.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OBJNERF_LIB") or os.path.join(_HERE, "csrc", "libobjnerf_hip.so")   # OBJNERF_LIB: diagnostic builds

OBJNERF_N_TENSORS = 19
ABI_VERSION = 14


class ObjnerfError(RuntimeError):
    pass


class Net(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("feat_dim", C.c_int32), ("n_freqs", C.c_int32),
                ("reserved", C.c_int32)]


class SampleArgs(C.Structure):
    _fields_ = [("F", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("n_frames", C.c_int32),
                ("n_px", C.c_int32), ("n_cam2surf", C.c_int32), ("n_bins", C.c_int32),
                ("obj_index", C.c_int32),
                ("surface_eps", C.c_float), ("stop_eps", C.c_float), ("min_bound", C.c_float),
                ("obj_center", C.c_float),
                ("rgbs", C.c_void_p), ("depth", C.c_void_p), ("t_wc", C.c_void_p), ("bbox", C.c_void_p),
                ("rays_dir_cache", C.c_void_p),
                ("kf_ids", C.c_void_p), ("u_w", C.c_void_p), ("u_h", C.c_void_p), ("u", C.c_void_p),
                ("g", C.c_void_p),
                ("out_rgb", C.c_void_p), ("out_depth", C.c_void_p), ("out_valid", C.c_void_p),
                ("out_labels", C.c_void_p), ("out_z", C.c_void_p), ("out_pts", C.c_void_p),
                ("max_depth_ws", C.c_void_p),
                ("seed", C.c_uint64), ("draw", C.c_uint32), ("reserved", C.c_uint32),
                ("kf_meta", C.c_void_p), ("out_kf", C.c_void_p), ("out_px", C.c_void_p),
                ("out_origins", C.c_void_p), ("out_dirs", C.c_void_p),
                # ABI 6: the part-feature gather (vmap.py:437-452)
                ("global_partfeat", C.c_void_p), ("use_frame", C.c_void_p), ("out_partfeat", C.c_void_p),
                ("pf_frames", C.c_int32), ("pf_w", C.c_int32), ("pf_h", C.c_int32), ("pf_c", C.c_int32),
                ("pf_stride", C.c_int32), ("part_down", C.c_float),
                # ABI 12: the gather through an index image (trailing, zero when not given: the dense form)
                ("part_index", C.c_void_p), ("pf_rows", C.c_int32), ("reserved_pf", C.c_int32)]


class IngestItem(C.Structure):
    _fields_ = [("rgbs", C.c_void_p), ("depth", C.c_void_p), ("t_wc", C.c_void_p), ("bbox", C.c_void_p),
                ("slot", C.c_int32), ("obj_id", C.c_int32), ("box", C.c_float * 4)]


class LossArgs(C.Structure):
    _fields_ = [("K", C.c_int32), ("R", C.c_int32), ("S", C.c_int32), ("C", C.c_int32),
                ("color_scaling", C.c_float), ("opacity_scaling", C.c_float),
                ("feat_scaling", C.c_float), ("reserved", C.c_float),
                ("alpha", C.c_void_p), ("color", C.c_void_p), ("z", C.c_void_p), ("gt_depth", C.c_void_p),
                ("gt_rgb", C.c_void_p), ("labels", C.c_void_p), ("pred_feat", C.c_void_p),
                ("gt_feat", C.c_void_p), ("flags_in", C.c_void_p), ("counts_in", C.c_void_p),
                ("loss_terms", C.c_void_p), ("total", C.c_void_p), ("d_alpha", C.c_void_p),
                ("d_color", C.c_void_p), ("d_pred_feat", C.c_void_p),
                ("counts", C.c_void_p), ("status", C.c_void_p)]


TRAIN_BF16 = 1       # objnerf_train_args.mode bit (OBJNERF_TRAIN_BF16)
TRAIN_SELF_COUNTS = 8    # (OBJNERF_TRAIN_SELF_COUNTS)


class AdamWArgs(C.Structure):
    _fields_ = [("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("group_steps", C.c_void_p),
                ("bank", C.c_int32), ("reserved", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("reserved_f", C.c_float)]


class TrainArgs(C.Structure):
    _fields_ = [("K", C.c_int32), ("R", C.c_int32), ("S", C.c_int32), ("mode", C.c_int32),
                ("color_scaling", C.c_float), ("opacity_scaling", C.c_float),
                ("feat_scaling", C.c_float), ("obj_center", C.c_float),
                ("params", C.c_void_p), ("p_stride", C.c_int64), ("scale", C.c_void_p),
                ("pts", C.c_void_p), ("origins", C.c_void_p), ("dirs", C.c_void_p), ("z", C.c_void_p),
                ("gt_depth", C.c_void_p), ("gt_rgb", C.c_void_p), ("labels", C.c_void_p),
                ("gt_feat", C.c_void_p),
                ("counts", C.c_void_p), ("flags", C.c_void_p),
                ("grads", C.c_void_p), ("loss_terms", C.c_void_p), ("status", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("relu_masks", C.c_void_p), ("context", C.c_void_p), ("emb_debug", C.c_void_p),
                ("optim", C.c_void_p)]


class KfStore(C.Structure):
    _fields_ = [("rgbs", C.c_void_p), ("depth", C.c_void_p), ("t_wc", C.c_void_p), ("bbox", C.c_void_p)]


class KfCrops(C.Structure):        # ABI 13: objnerf_kf_crops, a cropped keyframe store (kf_store.KeyframeCropStore)
    _fields_ = [("base", C.c_void_p), ("cap", C.c_int64), ("rect", C.c_void_p), ("t_wc", C.c_void_p),
                ("bbox", C.c_void_p)]


class IngestCropItem(C.Structure):
    _fields_ = [("store", KfCrops), ("slot", C.c_int32), ("obj_id", C.c_int32), ("box", C.c_float * 4),
                ("rect", C.c_int32 * 4)]


class VoxelArgs(C.Structure):
    _fields_ = [("K", C.c_int32), ("F", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("voxel", C.c_double),
                ("table", C.c_void_p), ("n_keyframes", C.c_void_p), ("camera_pose", C.c_void_p),
                ("crops", C.c_void_p)]      # ABI 13 (trailing; None = the dense tables)


class ObbArgs(C.Structure):
    _fields_ = [("K", C.c_int32), ("reserved", C.c_int32), ("verts", C.c_void_p), ("vert_off", C.c_void_p),
                ("normals", C.c_void_p), ("edges", C.c_void_p), ("cand", C.c_void_p), ("cand_off", C.c_void_p),
                ("mode", C.c_void_p)]


class ProjectArgs(C.Structure):
    _fields_ = [("S", C.c_int32), ("D", C.c_int32), ("Q", C.c_int32), ("flags", C.c_int32),
                ("V", C.c_int64), ("row_stride", C.c_int64),
                ("feat", C.c_void_p), ("seg_off", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p),
                ("out", C.c_void_p), ("minmax", C.c_void_p)]


class MomentsArgs(C.Structure):
    _fields_ = [("S", C.c_int32), ("D", C.c_int32), ("V", C.c_int64), ("row_stride", C.c_int64),
                ("feat", C.c_void_p), ("seg_off", C.c_void_p), ("mean", C.c_void_p), ("scatter", C.c_void_p)]


class ColorArgs(C.Structure):
    _fields_ = [("S", C.c_int32), ("Q", C.c_int32), ("V", C.c_int64), ("rgb_stride", C.c_int64),
                ("seg_off", C.c_void_p), ("mode", C.c_void_p), ("rgb", C.c_void_p), ("factor", C.c_void_p),
                ("constant", C.c_void_p), ("column", C.c_void_p), ("proj", C.c_void_p), ("minmax", C.c_void_p),
                ("out", C.c_void_p)]


class RayBoxesArgs(C.Structure):
    _fields_ = [("F", C.c_int32), ("N", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("depth", C.c_void_p), ("twc", C.c_void_p), ("boxes", C.c_void_p), ("out", C.c_void_p)]


class MaskPointsArgs(C.Structure):
    _fields_ = [("n", C.c_int64), ("W", C.c_int32), ("H", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("pix", C.c_void_p), ("depth", C.c_void_p), ("pose", C.c_void_p), ("out", C.c_void_p)]


class MapPointsHead(C.Structure):      # ABI 14: objnerf_mappoints_head_obj
    _fields_ = [("of_w", C.c_void_p), ("of_b", C.c_void_p), ("hfeat", C.c_void_p), ("row0", C.c_int64),
                ("H", C.c_int32), ("reserved", C.c_int32)]


class ViewHead(C.Structure):           # ABI 14: objnerf_view_head_obj
    _fields_ = [("of_w", C.c_void_p), ("of_b", C.c_void_p), ("hfeat", C.c_void_p), ("row0", C.c_int64),
                ("n_rows", C.c_int64), ("H", C.c_int32), ("reserved", C.c_int32)]


class AffinityArgs(C.Structure):
    _fields_ = [("N", C.c_int32), ("F", C.c_int32), ("d_cap", C.c_int32), ("d_clip", C.c_int32),
                ("w_geo", C.c_double), ("w_cap", C.c_double), ("w_clip", C.c_double), ("w_color", C.c_double),
                ("w_geo2d", C.c_double),
                ("boxes", C.c_void_p), ("cap", C.c_void_p), ("clip", C.c_void_p), ("color", C.c_void_p),
                ("boxes2d", C.c_void_p), ("W", C.c_void_p), ("terms", C.c_void_p)]


PROJ_COSINE = 1          # OBJNERF_PROJ_COSINE
PROJ_PER_SEGMENT = 2     # OBJNERF_PROJ_PER_SEGMENT
COLOR_RGB, COLOR_CONSTANT, COLOR_RAINBOW, COLOR_PCA = 0, 1, 2, 3      # OBJNERF_COLOR_*


# name -> (restype, argtypes); every symbol include/objnerf_hip.h declares
SIGNATURES = {
    "objnerf_abi_version": (C.c_int, []),
    "objnerf_context_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "objnerf_context_destroy": (C.c_int, [C.c_void_p]),
    "objnerf_param_layout": (C.c_int64, [C.POINTER(Net), C.POINTER(C.c_int64)]),
    "objnerf_rays_dirs": (C.c_int, [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p]),
    "objnerf_sample_rays": (C.c_int, [C.POINTER(SampleArgs), C.c_void_p]),
    "objnerf_sample_rays_stacked": (C.c_int, [C.POINTER(SampleArgs), C.c_int32, C.c_void_p, C.c_void_p]),
    "objnerf_sample_points": (C.c_int, [C.POINTER(SampleArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_ingest_frame": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p]),
    "objnerf_box_rays": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_box_points": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_render_fwd": (C.c_int, [C.POINTER(Net), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "objnerf_eval_points": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "objnerf_eval_workspace_bytes": (C.c_size_t, [C.POINTER(Net), C.c_int32, C.c_int64]),
    "objnerf_eval_points_ws": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "objnerf_mlp_forward": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "objnerf_mlp_forward_ws": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "objnerf_embed": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mlp_backward_workspace_bytes": (C.c_size_t, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_int32]),
    "objnerf_mlp_backward_ws": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "objnerf_embed_bwd": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_occupancy": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_render": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_render_loss": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "objnerf_reduce_batch_loss": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_make_grid": (C.c_int, [C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_ray_box": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "objnerf_dirs_w": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_stratified_bins": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p,
                                          C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
    "objnerf_normal_bins": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_void_p]),
    "objnerf_mfma_peak": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "objnerf_composite": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "objnerf_feature_head": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_step_batch_loss": (C.c_int, [C.POINTER(LossArgs), C.c_void_p]),
    "objnerf_label_counts": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "objnerf_train_workspace_bytes": (C.c_size_t, [C.POINTER(Net), C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int32]),
    "objnerf_train_step": (C.c_int, [C.POINTER(Net), C.POINTER(TrainArgs), C.c_void_p]),
    "objnerf_adamw_step": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float,
                                     C.c_float, C.c_float, C.c_void_p]),
    "objnerf_adamw_step_flags": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64,
                                           C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    # ABI 8: marching cubes (objnerf_mesh.hip)
    "objnerf_mc_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "objnerf_mc_count": (C.c_int, [C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "objnerf_mc_emit": (C.c_int, [C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mc_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ABI 9: object bounds from keyframes (objnerf_bounds.hip)
    "objnerf_voxel_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "objnerf_voxel_scan": (C.c_int, [C.POINTER(VoxelArgs), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_voxel_emit": (C.c_int, [C.POINTER(VoxelArgs), C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_voxel_heads_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "objnerf_voxel_heads": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_voxel_centroids": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_obb_search": (C.c_int, [C.POINTER(ObbArgs), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ABI 10: open-vocabulary queries over the exported map (objnerf_query.hip)
    "objnerf_project_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64]),
    "objnerf_project": (C.c_int, [C.POINTER(ProjectArgs), C.c_void_p, C.c_size_t, C.c_void_p]),
    "objnerf_moments_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "objnerf_moments": (C.c_int, [C.POINTER(MomentsArgs), C.c_void_p, C.c_size_t, C.c_void_p]),
    "objnerf_vertex_colors": (C.c_int, [C.POINTER(ColorArgs), C.c_void_p]),
    "objnerf_rainbow_lut": (C.c_int, [C.c_void_p]),
    # ABI 11: cross-frame mask association (objnerf_maskgraph.hip)
    "objnerf_cell_keys": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_dbscan_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "objnerf_dbscan": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "objnerf_cloud_overlap": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                        C.c_void_p, C.c_void_p]),
    "objnerf_mask_ray_boxes": (C.c_int, [C.POINTER(RayBoxesArgs), C.c_void_p]),
    "objnerf_mask_points": (C.c_int, [C.POINTER(MaskPointsArgs), C.c_void_p]),
    "objnerf_mask_hist": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "objnerf_point_bounds": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_affinity_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "objnerf_mask_affinity": (C.c_int, [C.POINTER(AffinityArgs), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "objnerf_mask_edges": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ABI 12: compact part-level feature maps (objnerf_partmap.hip)
    "objnerf_part_index": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_part_dense": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ABI 13: cropped keyframe stores (objnerf_misc.hip, objnerf_bounds.hip)
    "objnerf_ingest_frame_crops": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_sample_rays_crops": (C.c_int, [C.POINTER(SampleArgs), C.c_int32, C.c_void_p, C.c_void_p]),
    # ABI 14: labelling points against the whole map (objnerf_mappoints.hip)
    "objnerf_mappoints_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "objnerf_mappoints_count": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p]),
    "objnerf_mappoints_emit": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64,
                                         C.c_void_p, C.c_void_p]),
    "objnerf_mappoints_eval": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mappoints_gather": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "objnerf_mappoints_merge": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "objnerf_mappoints_resolve": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mappoints_head_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "objnerf_mappoints_head": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    # geometry evaluation (objnerf_mapeval.hip): additive, still ABI 14
    "objnerf_mesh_sample_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "objnerf_mesh_sample": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "objnerf_nearest_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "objnerf_nearest": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_seg_stats": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double),
                                    C.c_void_p, C.c_void_p]),
    # culling meshes to what the frames observed (objnerf_meshcull.hip): additive, still ABI 14
    "objnerf_vertex_views": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
                                       C.c_void_p, C.c_void_p]),
    "objnerf_mesh_cull_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "objnerf_mesh_cull_count": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mesh_cull_emit": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # a novel view of the whole map in one launch chain (objnerf_mapview.hip): additive, still ABI 14
    "objnerf_view_rays_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "objnerf_view_rays_count": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p]),
    "objnerf_view_rays_emit": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_render_fwd_segmented": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                               C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "objnerf_view_merge": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # part features and queries in a map view: additive, still ABI 14
    "objnerf_render_fwd_segmented_feat": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "objnerf_render_fwd_segmented_occupancy": (C.c_int, [C.c_int32]),
    "objnerf_view_query": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    # the compact exported map (objnerf_partrows.hip)
    "objnerf_part_rows": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "objnerf_part_expand": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    # scoring a rendered view against a frame (objnerf_vieweval.hip): additive, still ABI 14
    "objnerf_view_compare": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p]),
    # field gradients, nearest surface, rigid alignment (objnerf_mapalign.hip): additive, still ABI 14
    "objnerf_mappoints_grad": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "objnerf_embed_bwd_pts": (C.c_int, [C.POINTER(Net), C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mapalign_select": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                          C.c_void_p]),
    "objnerf_mapalign_resolve": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_mapalign_transform": (C.c_int, [C.c_int64, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "objnerf_mapalign_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "objnerf_mapalign_accumulate": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_double), C.c_double, C.c_double, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_void_p]),
    # the mask front end (objnerf_maskprep.hip): additive, still ABI 14
    "objnerf_cc_table_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "objnerf_cc_label": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_cc_table": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_cc_boundary": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "objnerf_cc_gaps": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p]),
    "objnerf_cc_relabel": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_clip_crops": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    # a navigation volume of the map (objnerf_mapvolume.hip): additive, still ABI 14
    "objnerf_volume_centres": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                         C.c_float, C.c_void_p, C.c_void_p]),
    "objnerf_volume_project": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_volume_clearance": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "objnerf_volume_reach_tiles": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "objnerf_volume_reach_rounds": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "objnerf_volume_goals": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "objnerf_volume_paths": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # part regions: connected patches of a part query on the meshes (objnerf_mapregions.hip): additive, still ABI 14
    "objnerf_regions_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int32]),
    "objnerf_regions_label": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_regions_table": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    # a rasteriser for the map's meshes (objnerf_mapraster.hip): additive, still ABI 14
    "objnerf_raster_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "objnerf_raster_visibility": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                            C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "objnerf_raster_resolve": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_double,
                                         C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # ray casting over the map's meshes (objnerf_maprays.hip): additive, still ABI 14
    "objnerf_rays_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "objnerf_rays_build": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "objnerf_rays_cast": (C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p,
                                    C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "objnerf_rays_resolve": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load (once) and return the library; raises ObjnerfError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ObjnerfError(
                f"{LIB_PATH} is missing: build it with `make -C openobj_amd/csrc` "
                "(or __graft_entry__.build()).  There is no CPU / PyTorch fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if l.objnerf_abi_version() != ABI_VERSION:
            raise ObjnerfError("libobjnerf_hip.so ABI version mismatch")
        _lib = l
    return _lib


_ERR = {-22: "EINVAL (bad shape / null pointer)", -95: "ENOTSUP (shape not built)",
        -5: "ELAUNCH (HIP launch failed)"}


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise ObjnerfError(f"{what} failed: {rc} {_ERR.get(rc, '')}")


def param_layout(hidden: int, feat_dim: int = 512, n_freqs: int = 6):
    """-> (offsets[20], p_stride)"""
    net = Net(hidden, feat_dim, n_freqs, 0)
    offs = (C.c_int64 * (OBJNERF_N_TENSORS + 1))()
    ps = lib().objnerf_param_layout(C.byref(net), offs)
    if ps < 0:
        raise ObjnerfError("objnerf_param_layout failed")
    return list(offs), int(ps)
