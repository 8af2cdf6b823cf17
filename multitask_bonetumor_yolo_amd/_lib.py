"""ctypes binding of libmtbt_hip.so (C ABI: include/mtbt_hip.h).  No fallback: a missing library is an error."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmtbt_hip.so")

ABI_VERSION = 5          # include/mtbt_hip.h MTBT_ABI_VERSION
F32, BF16, F16 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_ELU, ACT_GELU, ACT_GELU_POLY, ACT_DSILU, ACT_DELU, ACT_DGELU, ACT_DGELU_POLY = 0, 1, 2, 3, 4, 5, 6, 7, 8
OUT_NHWC, OUT_CONVT2X2 = 0, 1
RES_ID, RES_UP_BILINEAR, RES_DOWN_MEAN, RES_UP_NEAREST, RES_MAXPOOL = 0, 1, 2, 3, 4
CONFUSION_MAX_NC = 64    # include/mtbt_hip.h MTBT_CONFUSION_MAX_NC: classes of mtbt_det_confusion / mtbt_cls_confusion
WARP_CHUNK = 32          # csrc/warp_affine.hip MAX_CANVASES: canvases per launch of mtbt_warp_batch
WARP_LIN_MAX, WARP_OFF_MAX = 1 << 26, 1 << 47   # include/mtbt_hip.h mtbt_warp_batch: |a|, |b|, |d|, |e| and |c|, |f|
COPY_PASTE_CHUNK = 8     # csrc/copy_paste_check.h CHUNK: canvases per launch of mtbt_copy_paste
COPY_PASTE_MAX_ENTRIES = 16   # csrc/copy_paste_check.h MAX_ENTRIES: paste entries per canvas

ERRORS = {-1: "MTBT_EINVAL (bad argument / unsupported shape)", -2: "MTBT_EALIGN (misaligned pointer or stride)",
          -3: "MTBT_ELAUNCH (kernel launch failed)", -4: "MTBT_EWORKSPACE (workspace too small)"}


class ConvArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
        ("res", C.c_void_p),
        ("x_batch_stride", C.c_int64), ("y_batch_stride", C.c_int64), ("res_batch_stride", C.c_int64),
        ("x_pixel_stride", C.c_int32), ("y_pixel_stride", C.c_int32), ("res_pixel_stride", C.c_int32),
        ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("K", C.c_int32),
        ("R", C.c_int32), ("S", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("Ho", C.c_int32), ("Wo", C.c_int32), ("dtype", C.c_int32), ("out_dtype", C.c_int32),
        ("act", C.c_int32), ("out_mode", C.c_int32), ("tile_hint", C.c_int32), ("y2", C.c_void_p),
        ("policy", C.c_int32), ("debug", C.c_int32),
        ("colsum", C.c_void_p), ("colsum_shift", C.c_void_p), ("colsum_sq", C.c_int32), ("colsum_accumulate", C.c_int32),
        ("colsum_ws", C.c_void_p), ("colsum_ws_bytes", C.c_int64),
    ]


class FuseArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p * 3), ("wgt", C.c_float * 3), ("resample", C.c_int32 * 3), ("n_in", C.c_int32),
        ("y", C.c_void_p), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("dtype", C.c_int32), ("add_weight_bug", C.c_int32), ("wgt_dev", C.c_void_p),
    ]


class NodeArgs(C.Structure):  # mtbt_node_args
    _fields_ = [("fuse", FuseArgs), ("w", C.c_void_p), ("shift", C.c_void_p), ("y", C.c_void_p), ("y_pixel_stride", C.c_int32), ("K", C.c_int32),
                ("act", C.c_int32)]


class PwChainArgs(C.Structure):  # mtbt_pw_chain_args
    _fields_ = [("x", C.c_void_p), ("w1", C.c_void_p), ("scale1", C.c_void_p), ("shift1", C.c_void_p), ("w2", C.c_void_p), ("scale2", C.c_void_p),
                ("shift2", C.c_void_p), ("y", C.c_void_p), ("pixels", C.c_int64), ("y_pixel_stride", C.c_int32), ("C", C.c_int32), ("M", C.c_int32),
                ("K", C.c_int32), ("dtype", C.c_int32), ("out_dtype", C.c_int32), ("act1", C.c_int32), ("act2", C.c_int32)]


class UpconvArgs(C.Structure):  # mtbt_upconv_args
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p), ("shift", C.c_void_p),
                ("x_batch_stride", C.c_int64), ("y_batch_stride", C.c_int64), ("x_pixel_stride", C.c_int32), ("y_pixel_stride", C.c_int32),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("K", C.c_int32), ("dtype", C.c_int32), ("act", C.c_int32)]


class DecodeArgs(C.Structure):
    _fields_ = [
        ("map", C.c_void_p * 3), ("h", C.c_int32 * 3), ("w", C.c_int32 * 3), ("map_pixel_stride", C.c_int32 * 3),
        ("stride", C.c_float * 3), ("n_levels", C.c_int32), ("N", C.c_int32), ("nc", C.c_int32),
        ("reg_max", C.c_int32), ("xywh", C.c_int32),
        ("boxes", C.c_void_p), ("scores", C.c_void_p), ("best_score", C.c_void_p), ("best_label", C.c_void_p),
        ("preds_cat", C.c_void_p), ("cat_stride", C.c_int32),
    ]


class MaskArgs(C.Structure):
    _fields_ = [
        ("protos", C.c_void_p), ("coeff", C.c_void_p),
        ("coeff_batch_stride", C.c_int64), ("coeff_k_stride", C.c_int64), ("coeff_c_stride", C.c_int64),
        ("gather_idx", C.c_void_p), ("counts", C.c_void_p), ("bias", C.c_float),
        ("N", C.c_int32), ("K", C.c_int32), ("nm", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32),
        ("Hout", C.c_int32), ("Wout", C.c_int32), ("logits", C.c_void_p), ("masks", C.c_void_p),
    ]


class LossArgs(C.Structure):
    _fields_ = [
        ("map", C.c_void_p * 3), ("h", C.c_int32 * 3), ("w", C.c_int32 * 3), ("map_pixel_stride", C.c_int32 * 3),
        ("n_levels", C.c_int32), ("N", C.c_int32), ("nc", C.c_int32), ("reg_max", C.c_int32), ("img_size", C.c_float),
        ("gt_xyxy", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_off", C.c_void_p),
        ("iou_thresh", C.c_float), ("label_smoothing", C.c_float), ("training", C.c_int32),
        ("seg_logits", C.c_void_p), ("seg_targets", C.c_void_p), ("seg_bias", C.c_void_p), ("seg_n", C.c_int64),
        ("img_logits", C.c_void_p), ("img_gt", C.c_void_p), ("n_img_classes", C.c_int32),
        ("w_seg", C.c_float), ("w_box", C.c_float), ("w_dfl", C.c_float), ("w_cls", C.c_float), ("w_img", C.c_float),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out", C.c_void_p),
    ]


class BoxEvalArgs(C.Structure):  # mtbt_box_eval_args
    _fields_ = [("boxes", C.c_void_p), ("scores", C.c_void_p), ("labels", C.c_void_p), ("counts", C.c_void_p), ("gt", C.c_void_p),
                ("rank", C.c_void_p), ("match", C.c_void_p), ("ignore", C.c_void_p), ("gt_area", C.c_void_p), ("status", C.c_void_p),
                ("iou_thresholds", C.c_double * 32), ("B", C.c_int32), ("K", C.c_int32), ("M", C.c_int32), ("T", C.c_int32),
                ("max_det", C.c_int32), ("gt_format", C.c_int32), ("img_size", C.c_float)]


# every symbol include/mtbt_hip.h declares: name -> (restype, argtypes)
class PrepDesc(C.Structure):  # mtbt_prep_desc
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("scale0", C.c_void_p), ("scale1", C.c_void_p),
                ("sstride", C.c_int64 * 4), ("dim", C.c_int32 * 4), ("flip", C.c_int32 * 4),
                ("scale0_dim", C.c_int32), ("scale1_dim", C.c_int32), ("dst_dtype", C.c_int32), ("src_dim3", C.c_int32)]


class RawImage(C.Structure):  # mtbt_raw_image
    _fields_ = [("bgr", C.c_void_p), ("mask", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32),
                ("row_stride", C.c_int64), ("mask_row_stride", C.c_int64)]


class Frame(C.Structure):  # mtbt_frame
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("step", C.c_float), ("scale", C.c_float), ("pitch", C.c_int32),
                ("reserved", C.c_int32), ("offset", C.c_int64)]


class FrameMaskArgs(C.Structure):  # mtbt_frame_mask_args
    _fields_ = [("protos", C.c_void_p), ("coeff", C.c_void_p),
                ("coeff_batch_stride", C.c_int64), ("coeff_k_stride", C.c_int64), ("coeff_c_stride", C.c_int64),
                ("gather_idx", C.c_void_p), ("counts", C.c_void_p), ("boxes", C.c_void_p), ("boxes_frame", C.c_void_p),
                ("out", C.c_void_p), ("out_bytes", C.c_int64),
                ("N", C.c_int32), ("K", C.c_int32), ("nm", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32), ("crop", C.c_int32)]


class PackMasksArgs(C.Structure):  # mtbt_pack_masks_args
    _fields_ = [("src", C.c_void_p), ("plane_of", C.c_void_p), ("boxes", C.c_void_p), ("out", C.c_void_p),
                ("plane_stride", C.c_int64), ("row_stride", C.c_int64),
                ("n_src", C.c_int32), ("n_out", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32), ("dtype", C.c_int32)]


class MaskImage(C.Structure):  # mtbt_mask_image
    _fields_ = [("det", C.c_void_p), ("gt_base", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("g0", C.c_int32), ("gt_planes", C.c_int32), ("reserved", C.c_int32)]


class MaskPairArgs(C.Structure):  # mtbt_mask_pair_args
    _fields_ = [("counts", C.c_void_p), ("gt_image", C.c_void_p), ("inter", C.c_void_p), ("det_area", C.c_void_p), ("gt_area", C.c_void_p),
                ("B", C.c_int32), ("K", C.c_int32), ("M", C.c_int32), ("reserved", C.c_int32)]


class MaskEvalArgs(C.Structure):  # mtbt_mask_eval_args
    _fields_ = [("inter", C.c_void_p), ("det_area", C.c_void_p), ("gt_px", C.c_void_p), ("scores", C.c_void_p), ("labels", C.c_void_p),
                ("counts", C.c_void_p), ("gt_image", C.c_void_p), ("gt_label", C.c_void_p),
                ("rank", C.c_void_p), ("match", C.c_void_p), ("ignore", C.c_void_p), ("gt_area", C.c_void_p), ("status", C.c_void_p),
                ("iou_thresholds", C.c_double * 32), ("B", C.c_int32), ("K", C.c_int32), ("M", C.c_int32), ("T", C.c_int32),
                ("max_det", C.c_int32), ("reserved", C.c_int32)]


class MaskLossArgs(C.Structure):  # mtbt_mask_loss_args
    _fields_ = [("map", C.c_void_p * 3), ("h", C.c_int32 * 3), ("w", C.c_int32 * 3), ("map_pixel_stride", C.c_int32 * 3),
                ("n_levels", C.c_int32), ("N", C.c_int32), ("reg_max", C.c_int32), ("img_size", C.c_float), ("iou_thresh", C.c_float),
                ("n_gt", C.c_int32), ("gt_xyxy", C.c_void_p), ("gt_off", C.c_void_p), ("mc", C.c_void_p),
                ("mc_batch_stride", C.c_int64), ("mc_anchor_stride", C.c_int64), ("mc_channel_stride", C.c_int64),
                ("protos", C.c_void_p), ("gt_masks", C.c_void_p), ("hp", C.c_int32), ("wp", C.c_int32), ("nm", C.c_int32), ("weight", C.c_float),
                ("d_mc", C.c_void_p), ("d_protos", C.c_void_p), ("accumulate_dmc", C.c_int32), ("dprotos_dtype", C.c_int32),
                ("accumulate_dprotos", C.c_int32), ("reserved", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("out", C.c_void_p)]


class TalLossArgs(C.Structure):  # mtbt_tal_loss_args
    _fields_ = [("map", C.c_void_p * 3), ("h", C.c_int32 * 3), ("w", C.c_int32 * 3), ("map_pixel_stride", C.c_int32 * 3),
                ("n_levels", C.c_int32), ("N", C.c_int32), ("nc", C.c_int32), ("reg_max", C.c_int32), ("img_size", C.c_float),
                ("n_gt", C.c_int32), ("gt_xyxy", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_off", C.c_void_p),
                ("topk", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float), ("w_box", C.c_float), ("w_dfl", C.c_float), ("w_cls", C.c_float),
                ("accumulate", C.c_int32), ("reserved", C.c_int32), ("d_map", C.c_void_p * 3), ("d_map_pixel_stride", C.c_int32 * 3),
                ("reserved2", C.c_int32), ("assigned", C.c_void_p), ("target_score", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out", C.c_void_p)]


class BoxFuseArgs(C.Structure):  # mtbt_box_fuse_args (FuseArgs / mtbt_fuse_args is the BiFPN fusion node's)
    _fields_ = [("boxes", C.c_void_p * 8), ("scores", C.c_void_p * 8), ("labels", C.c_void_p * 8), ("counts", C.c_void_p * 8),
                ("anchors", C.c_void_p * 8), ("orient", C.c_int32 * 8), ("weight", C.c_float * 8),
                ("n_sources", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("top_k", C.c_int32),
                ("img_size", C.c_float), ("iou_thr", C.c_float), ("skip_thr", C.c_float), ("reserved", C.c_int32),
                ("out_boxes", C.c_void_p), ("out_scores", C.c_void_p), ("out_labels", C.c_void_p), ("out_counts", C.c_void_p),
                ("n_clusters", C.c_void_p), ("n_members", C.c_void_p), ("lead_source", C.c_void_p), ("lead_slot", C.c_void_p),
                ("lead_anchor", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class VoteMaskArgs(C.Structure):  # mtbt_vote_mask_args
    _fields_ = [("protos", C.c_void_p * 8), ("mc", C.c_void_p * 8),
                ("mc_batch_stride", C.c_int64 * 8), ("mc_k_stride", C.c_int64 * 8), ("mc_c_stride", C.c_int64 * 8),
                ("anchors", C.c_void_p * 8), ("scores", C.c_void_p * 8), ("weight", C.c_float * 8), ("orient", C.c_int32 * 8),
                ("member_slot", C.c_void_p), ("counts", C.c_void_p), ("boxes", C.c_void_p), ("boxes_frame", C.c_void_p),
                ("W", C.c_void_p), ("Ss", C.c_void_p), ("out", C.c_void_p), ("out_bytes", C.c_int64),
                ("n_sources", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("top_k", C.c_int32),
                ("nm", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32), ("crop", C.c_int32)]


class Tile(C.Structure):  # mtbt_tile
    _fields_ = [("image", C.c_int32), ("pox", C.c_int32), ("poy", C.c_int32),
                ("wx0", C.c_int32), ("wy0", C.c_int32), ("wx1", C.c_int32), ("wy1", C.c_int32),
                ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
                ("step", C.c_float), ("scale", C.c_float), ("fox", C.c_float), ("foy", C.c_float)]


class TileMergeArgs(C.Structure):  # mtbt_tile_merge_args
    _fields_ = [("boxes", C.c_void_p), ("scores", C.c_void_p), ("labels", C.c_void_p), ("counts", C.c_void_p), ("anchors", C.c_void_p),
                ("tiles", C.POINTER(Tile)), ("tiles_dev", C.c_void_p), ("first", C.POINTER(C.c_int32)),
                ("N", C.c_int32), ("n_tiles", C.c_int32), ("K", C.c_int32), ("top_k", C.c_int32),
                ("metric", C.c_int32), ("class_agnostic", C.c_int32), ("thr", C.c_float), ("skip_thr", C.c_float),
                ("out_boxes", C.c_void_p), ("out_scores", C.c_void_p), ("out_labels", C.c_void_p), ("out_counts", C.c_void_p),
                ("n_members", C.c_void_p), ("lead_tile", C.c_void_p), ("lead_slot", C.c_void_p), ("lead_anchor", C.c_void_p),
                ("member_slot", C.c_void_p), ("n_left", C.c_void_p)]


class TileMaskArgs(C.Structure):  # mtbt_tile_mask_args
    _fields_ = [("protos", C.c_void_p), ("mc", C.c_void_p),
                ("mc_batch_stride", C.c_int64), ("mc_k_stride", C.c_int64), ("mc_c_stride", C.c_int64),
                ("anchors", C.c_void_p), ("scores", C.c_void_p), ("member_slot", C.c_void_p), ("counts", C.c_void_p), ("boxes", C.c_void_p),
                ("tiles", C.POINTER(Tile)), ("tiles_dev", C.c_void_p), ("first", C.POINTER(C.c_int32)),
                ("W", C.c_void_p), ("Ss", C.c_void_p), ("out", C.c_void_p), ("out_bytes", C.c_int64),
                ("N", C.c_int32), ("n_tiles", C.c_int32), ("K", C.c_int32), ("top_k", C.c_int32), ("Tmax", C.c_int32),
                ("nm", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32), ("crop", C.c_int32), ("reserved", C.c_int32)]


class SegSource(C.Structure):  # mtbt_seg_source
    _fields_ = [("pass_", C.c_int32), ("slot", C.c_int32), ("orient", C.c_int32), ("proj", C.c_int32), ("blend", C.c_int32),
                ("weight", C.c_float), ("reserved", C.c_int32 * 2)]


class SegFrameArgs(C.Structure):  # mtbt_seg_frame_args
    _fields_ = [("protos", C.c_void_p * 64), ("pass_items", C.c_int32 * 64), ("proj", C.c_void_p),
                ("sources", C.POINTER(SegSource)), ("sources_dev", C.c_void_p),
                ("tiles", C.POINTER(Tile)), ("tiles_dev", C.c_void_p), ("first", C.POINTER(C.c_int32)),
                ("tab", C.POINTER(C.c_float)), ("tab_dev", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out", C.c_void_p), ("out_bytes", C.c_int64),
                ("logits", C.c_void_p), ("logits_floats", C.c_int64), ("logits_offset", C.c_int64 * 32), ("threshold", C.c_float),
                ("N", C.c_int32), ("n_sources", C.c_int32), ("n_passes", C.c_int32), ("n_proj", C.c_int32),
                ("nm", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32), ("reserved", C.c_int32)]


class SurfaceArgs(C.Structure):  # mtbt_surface_args
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("n_edge", C.c_void_p), ("max_d2", C.c_void_p), ("n_within", C.c_void_p), ("sum_d", C.c_void_p), ("rank_d2", C.c_void_p),
                ("q", C.c_double * 4), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("tol2", C.c_uint32), ("Q", C.c_int32)]


class ComponentsArgs(C.Structure):  # mtbt_components_args
    _fields_ = [("packed", C.c_void_p), ("other", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("labels", C.c_void_p), ("n_components", C.c_void_p), ("area", C.c_void_p), ("box", C.c_void_p), ("first", C.c_void_p),
                ("inter", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("connectivity", C.c_int32), ("max_components", C.c_int32)]


class SelectComponentsArgs(C.Structure):  # mtbt_select_components_args
    _fields_ = [("packed", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out", C.c_void_p),
                ("n_kept", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("min_area", C.c_uint32), ("keep_largest", C.c_int32)]


class FillPolygonsArgs(C.Structure):  # mtbt_fill_polygons_args
    _fields_ = [("vertices", C.c_void_p), ("poly_offsets", C.c_void_p), ("plane_offsets", C.c_void_p), ("clip", C.c_void_p),
                ("out", C.c_void_p), ("area", C.c_void_p), ("box", C.c_void_p),
                ("n", C.c_int32), ("n_polys", C.c_int32), ("n_vertices", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32)]


class ClaheImage(C.Structure):  # mtbt_clahe_image
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("clip", C.c_int32),
                ("src_row_stride", C.c_int64), ("dst_row_stride", C.c_int64)]


class CopyPasteArgs(C.Structure):  # mtbt_copy_paste_args
    _fields_ = [("images", C.c_void_p), ("planes", C.c_void_p), ("rows_in", C.c_void_p),
                ("row_off", C.POINTER(C.c_int32)), ("paste_off", C.POINTER(C.c_int32)), ("entries", C.POINTER(C.c_int32)),
                ("out_images", C.c_void_p), ("out_planes", C.c_void_p), ("out_masks", C.c_void_p), ("rows_out", C.c_void_p),
                ("area_before", C.c_void_p), ("area", C.c_void_p), ("box", C.c_void_p),
                ("B", C.c_int32), ("M", C.c_int32), ("P", C.c_int32), ("S", C.c_int32), ("pitch", C.c_int32), ("entry_stride", C.c_int32)]


class DistanceTransformArgs(C.Structure):  # mtbt_distance_transform_args
    _fields_ = [("packed", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("d2_set", C.c_void_p),
                ("d2_unset", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32)]


class SegRegionArgs(C.Structure):  # mtbt_seg_region_args
    _fields_ = [("logits", C.c_void_p), ("bias", C.c_void_p), ("targets", C.c_void_p), ("d2_set", C.c_void_p), ("d2_unset", C.c_void_p),
                ("d_logits", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("out", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("smooth", C.c_float), ("w_dice", C.c_float), ("w_boundary", C.c_float), ("accumulate", C.c_int32)]


class ContoursArgs(C.Structure):  # mtbt_contours_args
    _fields_ = [("packed", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("n_vertices", C.c_void_p),
                ("n_contours", C.c_void_p), ("vertices", C.c_void_p), ("offset", C.c_void_p), ("count", C.c_void_p), ("area2", C.c_void_p),
                ("box", C.c_void_p), ("start", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("connectivity", C.c_int32), ("max_contours", C.c_int32), ("max_vertices", C.c_int32), ("reserved", C.c_int32)]


class RleArgs(C.Structure):  # mtbt_rle_args
    _fields_ = [("packed", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64), ("counts", C.c_void_p),
                ("n_runs", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("max_runs", C.c_int32), ("reserved", C.c_int32)]


class MeasureArgs(C.Structure):  # mtbt_measure_args
    _fields_ = [("packed", C.c_void_p), ("labels", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
                ("sums", C.c_void_p), ("n_hull", C.c_void_p), ("hull", C.c_void_p), ("hull_area2", C.c_void_p), ("caliper", C.c_void_p),
                ("caliper_at", C.c_void_p), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pitch", C.c_int32),
                ("max_regions", C.c_int32), ("max_hull", C.c_int32), ("reserved", C.c_int32 * 2)]


SYMBOLS = {
    "mtbt_abi_version": (C.c_int, []),
    "mtbt_sizeof_args": (C.c_int, [C.c_int]),
    "mtbt_target_arch": (C.c_char_p, []),
    "mtbt_conv2d_nhwc": (C.c_int, [C.POINTER(ConvArgs), C.c_void_p]),
    "mtbt_convt2x2_conv3x3_nhwc": (C.c_int, [C.POINTER(UpconvArgs), C.c_void_p]),
    "mtbt_stem_conv4x4_ln": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "mtbt_dwconv_nhwc": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
                         + [C.c_int] * 6 + [C.c_void_p]),
    "mtbt_layernorm_nhwc": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_bifpn_fuse": (C.c_int, [C.POINTER(FuseArgs), C.c_void_p]),
    "mtbt_bifpn_node_nhwc": (C.c_int, [C.POINTER(NodeArgs), C.c_void_p]),
    "mtbt_pw_chain_nhwc": (C.c_int, [C.POINTER(PwChainArgs), C.c_void_p]),
    "mtbt_pw_chain_supported": (C.c_int, [C.POINTER(PwChainArgs)]),
    "mtbt_sizeof_pw_chain_args": (C.c_int, []),
    "mtbt_bn_train_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "mtbt_bn_train_nhwc": (C.c_int, [C.c_void_p] * 6 + [C.c_float, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                      C.c_int64, C.c_void_p]),
    "mtbt_gap_fc": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_void_p]),
    "mtbt_decode_boxes": (C.c_int, [C.POINTER(DecodeArgs), C.c_void_p]),
    "mtbt_nms_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "mtbt_nms_batched": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]
                         + [C.c_void_p] * 8 + [C.c_int64, C.c_void_p]),
    "mtbt_mask_assemble": (C.c_int, [C.POINTER(MaskArgs), C.c_void_p]),
    "mtbt_loss_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int64]),
    "mtbt_multitask_loss": (C.c_int, [C.POINTER(LossArgs), C.c_void_p]),
    "mtbt_multitask_loss_grad": (C.c_int, [C.POINTER(LossArgs), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_convnext_mlp_fused": (C.c_int, [C.c_void_p] * 7 + [C.c_int64, C.c_int, C.c_void_p]),
    "mtbt_convnext_mlp_fused_dt": (C.c_int, [C.c_void_p] * 7 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_convnext_mlp_fused_train": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_void_p]),
    "mtbt_bbox_iou_pairwise": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "mtbt_letterbox_batch": (C.c_int, [C.POINTER(RawImage), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "mtbt_augment_batch": (C.c_int, [C.POINTER(RawImage), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_mosaic_batch": (C.c_int, [C.POINTER(RawImage), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_warp_batch": (C.c_int, [C.POINTER(RawImage), C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_seg_confusion_workspace_bytes": (C.c_int64, [C.c_int]),
    "mtbt_seg_confusion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_conv_wgrad_workspace_bytes": (C.c_int64, [C.c_int] * 7),
    "mtbt_conv_wgrad": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 9 + [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_void_p,
                                  C.c_int64, C.c_void_p]),
    "mtbt_conv_wgrad_xact": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 9 + [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_int64, C.c_void_p]),
    "mtbt_conv_wgrad_bias": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 9 + [C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int, C.c_int, C.c_void_p,
                                       C.c_int64, C.c_void_p]),
    "mtbt_act_backward": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_channel_sum_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "mtbt_channel_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_int64, C.c_void_p]),
    "mtbt_channel_affine2": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_layernorm_backward_nhwc": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_layernorm_backward_params_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "mtbt_layernorm_backward_params_nhwc": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_dwconv_wgrad_workspace_bytes": (C.c_int64, [C.c_int] * 5),
    "mtbt_dwconv_wgrad": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 7 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_dwconv_wgrad_bias": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_adamw_step": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_float] * 5 + [C.c_int64, C.c_void_p, C.c_void_p]),
    "mtbt_sgd_step": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_float] * 4 + [C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "mtbt_adamw_step_ema": (C.c_int, [C.c_void_p] * 5 + [C.c_int64] + [C.c_float] * 5 + [C.c_int64, C.c_void_p, C.c_double, C.c_void_p]),
    "mtbt_sgd_step_ema": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_float] * 4 + [C.c_int, C.c_int64, C.c_void_p, C.c_double, C.c_void_p]),
    "mtbt_ema_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]),
    "mtbt_sumsq_workspace_bytes": (C.c_int64, []),
    "mtbt_sumsq": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_clip_coef": (C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_stem_conv4x4_ln_train": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "mtbt_dwconv_nhwc_train": (C.c_int, [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
                               + [C.c_int] * 6 + [C.c_void_p]),
    "mtbt_bn_forward_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_bn_forward_sums_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_conv_colsum_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "mtbt_conv_colsum_layout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_conv_kernel_choice": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mtbt_conv2d_nhwc_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mtbt_conv_batch_kernel_choice": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mtbt_dwconv3x3_mult_nhwc": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]),
    "mtbt_dwconv_kernel_choice": (C.c_int, [C.c_int] * 8 + [C.c_void_p]),
    "mtbt_dwconv3x3_mult_kernel_choice": (C.c_int, [C.c_int] * 7 + [C.c_void_p]),
    "mtbt_bn_forward_partials_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_int, C.c_int64, C.c_int, C.c_int,
                                                C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_bn_backward_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "mtbt_bn_backward_nhwc": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 3
                              + [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_weight_prep_blocks": (C.c_int, [C.c_int64]),
    "mtbt_weight_prep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_bifpn_norm_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "mtbt_bifpn_norm_weights_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mtbt_wadd_norm_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "mtbt_wadd_norm_weights_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "mtbt_resample_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 5 + [C.c_void_p]),
    "mtbt_bifpn_fuse_backward_workspace_bytes": (C.c_int64, []),
    "mtbt_bifpn_fuse_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 5
                                 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_projector_backward_workspace_bytes": (C.c_int64, [C.c_int] * 4),
    "mtbt_projector_backward": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_int] * 6
                                + [C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_gap_fc_backward": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "mtbt_copy_strided": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.c_int, C.c_int64, C.c_int32, C.c_int, C.c_int64,
                                    C.c_int, C.c_int, C.c_void_p]),
    "mtbt_scale_grad": (C.c_int, [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_add_nhwc": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_stem_wgrad_workspace_bytes": (C.c_int64, [C.c_int]),
    "mtbt_stem_wgrad": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_cast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "mtbt_box_eval": (C.c_int, [C.POINTER(BoxEvalArgs), C.c_void_p]),
    "mtbt_det_confusion": (C.c_int, [C.POINTER(LossArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_cls_confusion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mtbt_masks_to_frames": (C.c_int, [C.POINTER(FrameMaskArgs), C.POINTER(Frame), C.c_int, C.c_void_p]),
    "mtbt_sizeof_frame_args": (C.c_int, [C.c_int]),
    "mtbt_pack_masks": (C.c_int, [C.POINTER(PackMasksArgs), C.c_void_p]),
    "mtbt_mask_pair_counts": (C.c_int, [C.POINTER(MaskPairArgs), C.POINTER(MaskImage), C.c_int, C.c_void_p]),
    "mtbt_mask_eval": (C.c_int, [C.POINTER(MaskEvalArgs), C.c_void_p]),
    "mtbt_sizeof_mask_eval_args": (C.c_int, [C.c_int]),
    "mtbt_mask_loss_workspace_bytes": (C.c_int64, [C.c_int] * 5),
    "mtbt_instance_mask_loss": (C.c_int, [C.POINTER(MaskLossArgs), C.c_void_p]),
    "mtbt_instance_mask_loss_assigned": (C.c_int, [C.POINTER(MaskLossArgs), C.c_void_p, C.c_void_p]),
    "mtbt_sizeof_mask_loss_args": (C.c_int, []),
    "mtbt_tal_loss_workspace_bytes": (C.c_int64, [C.c_int] * 3),
    "mtbt_tal_det_loss": (C.c_int, [C.POINTER(TalLossArgs), C.c_void_p]),
    "mtbt_sizeof_tal_loss_args": (C.c_int, []),
    "mtbt_fuse_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mtbt_fuse_detections": (C.c_int, [C.POINTER(BoxFuseArgs), C.c_void_p]),
    "mtbt_sizeof_box_fuse_args": (C.c_int, []),
    "mtbt_fuse_detections_members": (C.c_int, [C.POINTER(BoxFuseArgs), C.c_void_p, C.c_void_p]),
    "mtbt_vote_masks": (C.c_int, [C.POINTER(VoteMaskArgs), C.POINTER(Frame), C.c_int, C.c_void_p]),
    "mtbt_sizeof_vote_mask_args": (C.c_int, []),
    "mtbt_merge_tiles": (C.c_int, [C.POINTER(TileMergeArgs), C.c_void_p]),
    "mtbt_vote_tile_masks": (C.c_int, [C.POINTER(TileMaskArgs), C.POINTER(Frame), C.c_int, C.c_void_p]),
    "mtbt_sizeof_tile_args": (C.c_int, [C.c_int]),
    "mtbt_seg_to_frames": (C.c_int, [C.POINTER(SegFrameArgs), C.POINTER(Frame), C.c_int, C.c_void_p]),
    "mtbt_seg_frame_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "mtbt_sizeof_seg_frame_args": (C.c_int, [C.c_int]),
    "mtbt_surface_distances_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mtbt_surface_distances": (C.c_int, [C.POINTER(SurfaceArgs), C.c_void_p]),
    "mtbt_sizeof_surface_args": (C.c_int, [C.c_int]),
    "mtbt_components_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mtbt_label_components": (C.c_int, [C.POINTER(ComponentsArgs), C.c_void_p]),
    "mtbt_select_components": (C.c_int, [C.POINTER(SelectComponentsArgs), C.c_void_p]),
    "mtbt_sizeof_components_args": (C.c_int, [C.c_int]),
    "mtbt_fill_polygons": (C.c_int, [C.POINTER(FillPolygonsArgs), C.c_void_p]),
    "mtbt_sizeof_fill_polygons_args": (C.c_int, [C.c_int]),
    "mtbt_clahe_workspace_bytes": (C.c_int64, [C.POINTER(ClaheImage), C.c_int, C.c_int, C.c_int]),
    "mtbt_clahe_batch": (C.c_int, [C.POINTER(ClaheImage), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mtbt_sizeof_clahe_args": (C.c_int, [C.c_int]),
    "mtbt_copy_paste": (C.c_int, [C.POINTER(CopyPasteArgs), C.c_void_p]),
    "mtbt_sizeof_copy_paste_args": (C.c_int, [C.c_int]),
    "mtbt_distance_transform_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mtbt_distance_transform": (C.c_int, [C.POINTER(DistanceTransformArgs), C.c_void_p]),
    "mtbt_seg_region_loss_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mtbt_seg_region_loss": (C.c_int, [C.POINTER(SegRegionArgs), C.c_void_p]),
    "mtbt_sizeof_distance_args": (C.c_int, [C.c_int]),
    "mtbt_contours_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mtbt_trace_contours": (C.c_int, [C.POINTER(ContoursArgs), C.c_void_p]),
    "mtbt_rle_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mtbt_rle_encode": (C.c_int, [C.POINTER(RleArgs), C.c_void_p]),
    "mtbt_sizeof_contours_args": (C.c_int, [C.c_int]),
    "mtbt_measure_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mtbt_measure_regions": (C.c_int, [C.POINTER(MeasureArgs), C.c_void_p]),
    "mtbt_sizeof_measure_args": (C.c_int, [C.c_int]),
}

ARG_STRUCTS = (ConvArgs, FuseArgs, DecodeArgs, MaskArgs, LossArgs, PrepDesc, RawImage, UpconvArgs, NodeArgs, BoxEvalArgs)   # order of mtbt_sizeof_args(which)
FRAME_STRUCTS = (Frame, FrameMaskArgs)   # order of mtbt_sizeof_frame_args(which)
MASK_EVAL_STRUCTS = (PackMasksArgs, MaskImage, MaskPairArgs, MaskEvalArgs)   # order of mtbt_sizeof_mask_eval_args(which)
TILE_STRUCTS = (Tile, TileMergeArgs, TileMaskArgs)   # order of mtbt_sizeof_tile_args(which)
SEG_FRAME_STRUCTS = (SegSource, SegFrameArgs)   # order of mtbt_sizeof_seg_frame_args(which)
SURFACE_STRUCTS = (SurfaceArgs,)   # order of mtbt_sizeof_surface_args(which)
COMPONENTS_STRUCTS = (ComponentsArgs, SelectComponentsArgs)   # order of mtbt_sizeof_components_args(which)
POLYGON_STRUCTS = (FillPolygonsArgs,)   # order of mtbt_sizeof_fill_polygons_args(which)
CLAHE_STRUCTS = (ClaheImage,)   # order of mtbt_sizeof_clahe_args(which)
COPY_PASTE_STRUCTS = (CopyPasteArgs,)   # order of mtbt_sizeof_copy_paste_args(which)
DISTANCE_STRUCTS = (DistanceTransformArgs, SegRegionArgs)   # order of mtbt_sizeof_distance_args(which)
CONTOURS_STRUCTS = (ContoursArgs, RleArgs)   # order of mtbt_sizeof_contours_args(which)
MEASURE_STRUCTS = (MeasureArgs,)   # order of mtbt_sizeof_measure_args(which)
_lib = None


def load():
    """Load the HIP library or raise: the product has no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -m multitask_bonetumor_yolo_amd.build` "
                               "(there is no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.mtbt_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libmtbt_hip.so reports ABI version {lib.mtbt_abi_version()}, this binding is version {ABI_VERSION}: rebuild "
                               "(`python -m multitask_bonetumor_yolo_amd.build`)")
        for which, st in enumerate(ARG_STRUCTS):
            if lib.mtbt_sizeof_args(which) != C.sizeof(st):
                raise RuntimeError(f"libmtbt_hip.so was built with sizeof({st.__name__}) = {lib.mtbt_sizeof_args(which)}, this binding lays it out in "
                                   f"{C.sizeof(st)} bytes: stale library, rebuild")
        for sizeof, structs in ((lib.mtbt_sizeof_frame_args, FRAME_STRUCTS), (lib.mtbt_sizeof_mask_eval_args, MASK_EVAL_STRUCTS),
                                (lib.mtbt_sizeof_tile_args, TILE_STRUCTS), (lib.mtbt_sizeof_surface_args, SURFACE_STRUCTS),
                                (lib.mtbt_sizeof_components_args, COMPONENTS_STRUCTS), (lib.mtbt_sizeof_fill_polygons_args, POLYGON_STRUCTS),
                                (lib.mtbt_sizeof_clahe_args, CLAHE_STRUCTS), (lib.mtbt_sizeof_copy_paste_args, COPY_PASTE_STRUCTS),
                                (lib.mtbt_sizeof_distance_args, DISTANCE_STRUCTS), (lib.mtbt_sizeof_seg_frame_args, SEG_FRAME_STRUCTS),
                                (lib.mtbt_sizeof_contours_args, CONTOURS_STRUCTS), (lib.mtbt_sizeof_measure_args, MEASURE_STRUCTS)):
            for which, st in enumerate(structs):
                if sizeof(which) != C.sizeof(st):
                    raise RuntimeError(f"libmtbt_hip.so was built with sizeof({st.__name__}) = {sizeof(which)}, this binding lays it "
                                       f"out in {C.sizeof(st)} bytes: stale library, rebuild")
        for sizeof, st in ((lib.mtbt_sizeof_mask_loss_args, MaskLossArgs), (lib.mtbt_sizeof_tal_loss_args, TalLossArgs),
                           (lib.mtbt_sizeof_pw_chain_args, PwChainArgs), (lib.mtbt_sizeof_box_fuse_args, BoxFuseArgs),
                           (lib.mtbt_sizeof_vote_mask_args, VoteMaskArgs)):
            if sizeof() != C.sizeof(st):
                raise RuntimeError(f"libmtbt_hip.so was built with sizeof({st.__name__}) = {sizeof()}, this binding lays it "
                                   f"out in {C.sizeof(st)} bytes: stale library, rebuild")
        _lib = lib
    return _lib


def check(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what}: {ERRORS.get(code, code)}")


def stream(dev):
    """The current stream of `dev`, as the `void* stream` every entry point takes last."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(fn, *dims, device, what: str):
    """The scratch buffer a `*_workspace_bytes` query `fn(*dims)` asks for -> (uint8 tensor, nbytes).  A negative answer is the query's
    refusal of the shape and raises through `check` under the name `what`; the tensor has at least 16 bytes, so that it has an address."""
    nbytes = int(fn(*dims))
    if nbytes < 0:
        check(nbytes, what)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device), nbytes
