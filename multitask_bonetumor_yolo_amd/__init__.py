"""MI355X-native multitask YOLO hot path: drop-in ConvNeXtBiFPNYOLO over hand-written HIP kernels.

    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO          # == reference main_model.ConvNeXtBiFPNYOLO
    from multitask_bonetumor_yolo_amd import postprocess                 # decode / NMS / masks on the GPU
    from multitask_bonetumor_yolo_amd import preprocess                  # letterbox / BGR->RGB / /255 of a batch on the GPU
    from multitask_bonetumor_yolo_amd import planes                      # bit-packed mask planes: pack, components, distances, polygons, RLE
    from multitask_bonetumor_yolo_amd import augment_samples             # training augmentation fused into that launch (the reference has none)
    from multitask_bonetumor_yolo_amd import mosaic_samples              # the same with four images per canvas
    from multitask_bonetumor_yolo_amd import affine_samples, affine_samples_seg   # rotation and shear: an affine map per canvas, labels moved with it
    from multitask_bonetumor_yolo_amd import multitask_loss              # == MultiTaskLitModel._multitask_loss (value)
    from multitask_bonetumor_yolo_amd import instance_mask_loss          # YOLOv8-seg instance-mask loss + gradients (opt-in extension)
    from multitask_bonetumor_yolo_amd import task_aligned_det_loss       # task-aligned (YOLOv8) detection loss + gradients (opt-in extension)
    from multitask_bonetumor_yolo_amd import TaskAlignedSegLoss          # both in one autograd node: the mask term on the task-aligned assignment
    from multitask_bonetumor_yolo_amd import ValidationStep              # == validation_step + the epoch-end metrics, on the device
    from multitask_bonetumor_yolo_amd import TrainStep, ema_decay_at     # the native training step (ema=: averaged weights in the optimiser pass)
    from multitask_bonetumor_yolo_amd import save_train_state, load_train_state   # stop a TrainStep and continue it
    from multitask_bonetumor_yolo_amd import detect_fused                # test-time augmentation / ensembles: weighted boxes fusion on the device
    from multitask_bonetumor_yolo_amd import vote_masks                  # instance masks of a fused list, voted over each cluster's members
    from multitask_bonetumor_yolo_amd import detect_sliced               # sliced inference: tiles of a large image, merged and voted on the device
    from multitask_bonetumor_yolo_amd import SurfaceDistanceMetrics      # Hausdorff / HD95 / ASSD / surface Dice from packed masks, on the device
    from multitask_bonetumor_yolo_amd import label_components, LesionMetrics   # connected components of packed masks; lesion-wise recall / precision
    from multitask_bonetumor_yolo_amd import fill_polygons, yolo_seg_planes, augment_samples_seg   # polygon labels -> packed instance masks
    from multitask_bonetumor_yolo_amd import clahe_batch                 # tile-wise contrast equalisation (CLAHE) of the raw uint8 images
    from multitask_bonetumor_yolo_amd import copy_paste_batch, sample_copy_paste   # instances pasted between the canvases of a batch
    from multitask_bonetumor_yolo_amd import distance_transform, signed_distance   # exact Euclidean distance maps of packed masks
    from multitask_bonetumor_yolo_amd import seg_region_loss, SegRegionLoss   # soft Dice + boundary terms of the segmentation loss
    from multitask_bonetumor_yolo_amd import trace_contours, yolo_seg_rows, labelme_shapes   # packed masks -> polygons (YOLO-seg rows, LabelMe shapes)
    from multitask_bonetumor_yolo_amd import rle_encode, coco_segm_results   # packed masks -> COCO run lengths and a segm results list
    from multitask_bonetumor_yolo_amd import measure_regions, region_properties, measure_detections   # hull, Feret diameters, moments of lesions

The HIP library (csrc/libmtbt_hip.so, C ABI in include/mtbt_hip.h) is built by
`python -m multitask_bonetumor_yolo_amd.build`; nothing here falls back to the CPU.
"""
from . import planes, postprocess, preprocess  # noqa: F401
from .preprocess import (affine_coefficients, affine_forward, affine_polygons, affine_samples, affine_samples_seg, affine_yolo_labels,  # noqa: F401
                         sample_affine, warp_batch)
from .preprocess import copy_paste_batch, sample_copy_paste  # noqa: F401
from .preprocess import (augment_batch, augment_polygons, augment_samples, augment_samples_seg, augment_yolo_labels, clahe_batch, clahe_clip,  # noqa: F401
                         letterbox_geometry, mosaic_batch, mosaic_polygons, mosaic_samples, mosaic_samples_seg, mosaic_yolo_labels, photometric_lut,
                         sample_clahe, sample_geometry, sample_mosaic, sample_photometric, slice_batch, slice_geometry)
from .loss import (InstanceMaskLoss, SegRegionLoss, TaskAlignedDetLoss, TaskAlignedSegLoss, instance_mask_loss, multitask_loss,  # noqa: F401
                   seg_region_loss, task_aligned_det_loss)
from .checkpoints import load_pretrained_heads, load_train_state, save_train_state, strip_lightning_prefix  # noqa: F401
from .graphed import GraphedInference  # noqa: F401
from .metrics import (DetectionConfusionMatrix, DeviceMaskMeanAveragePrecision, DeviceMeanAveragePrecision,  # noqa: F401
                      ImageClassificationMetrics, LesionMetrics, MeanAveragePrecision, SegmentationMetrics, SurfaceDistanceMetrics,
                      lesion_hits, surface_distances, surface_metrics)
from .validate import ValidationStep  # noqa: F401
from .ensemble import detect_fused  # noqa: F401
from .postprocess import merge_tiles, seg_to_frames, vote_masks, vote_tile_masks  # noqa: F401
from .planes import (coco_segm_results, components_to_instances, contour_polygons, count_contour_vertices, distance_transform, fill_polygons,  # noqa: F401
                     filter_components, label_components, labelme_shapes, measure_components, measure_detections, measure_regions,
                     region_properties, rle_encode, rle_from_string, rle_to_string, signed_distance, trace_contours, yolo_seg_planes,
                     yolo_seg_polygons, yolo_seg_rows)
from .sliced import detect_sliced  # noqa: F401
from .trainstep import TrainStep, ema_decay_at  # noqa: F401
from .model import ConvNeXtBiFPNYOLO, ConvNeXtBiFPNYOLOv0, ConvNeXtBiFPNYOLOv2, calibrate_synthetic_heads_, init_synthetic_, synthetic_images  # noqa: F401
