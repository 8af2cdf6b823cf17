"""CPU checks of csrc/bitplane.h, the one place that holds the layout of a bit-packed plane: its host half as a stand-alone program
(tests/bitplane_check_main.cpp) built by a plain host compiler and under the address and undefined-behaviour sanitizers, the shapes the
library's entry points accept, and the Python side of the same move (planes.py; every name where it was importable from before).

The accepted shapes below are data, written down from the conditions the entry points had when each spelled its own:
  dims        n >= 0, 1 <= H, W <= 16384, pitch == 8 * ceil(W / 64)          surface distances, distance transform, region loss, contours, RLE
  components  the same and H * W < 2^31 (which 16384^2 = 2^28 never reaches)
  area        H, W >= 1, H * W < 2^31, the pitch rule, no 16384                mask_eval.hip, polygon_fill.hip
  square      S >= 4, S % 4 == 0, S <= 32768, pitch == 8 * ceil(S / 64)       copy_paste_check.h
"""
import os
import re
import shutil
import subprocess

import pytest

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH = {1: 8, 63: 8, 64: 8, 65: 16, 127: 16, 128: 16, 129: 24, 16384: 2048, 16385: 2056}   # by hand: 1, 1, 1, 2, 2, 2, 3, 256, 257 words
WS, HS = (1, 63, 64, 65, 127, 128, 129, 16384, 16385), (1, 16384, 16385)
DIMS = {(H, W, PITCH[W]) for H in (1, 16384) for W in WS[:-1]}
ACCEPTED = {
    "dims": DIMS,
    "components": DIMS,
    "area": {(H, W, PITCH[W]) for H in HS for W in WS} | {(32768, 65535, 8192)},    # 2^31 - 32768 pixels; 32768 x 65536 = 2^31 is refused
    "square": {(1, 64, 8), (1, 128, 16), (1, 16384, 2048)},
}


def _run_program(tmp_path, compiler, flags):
    exe = str(tmp_path / "bitplane_check")
    cmd = [compiler, "-std=c++17", "-O1", "-g", *flags, "-I" + B.INCLUDE, "-I" + B.CSRC, os.path.join(ROOT, "tests", "bitplane_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"bitplane_check: \d+ cases ok", r.stdout), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = {k: set() for k in ACCEPTED}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] in got:
            got[f[0]].add(tuple(int(v) for v in f[1:]))
    return got


def test_host_half_accepts_what_the_entry_points_accepted_under_sanitizers(tmp_path):
    got = _run_program(tmp_path, B.HIPCC, ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    for family, want in ACCEPTED.items():
        assert got[family] == want, (family, sorted(got[family] ^ want))


def test_host_half_needs_no_hip(tmp_path):
    """copy_paste_check.h, and through it bitplane.h, are plain C++: the same program from the host compiler alone."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(B.HIPCC)))
    found = [shutil.which(c) for c in ("g++", "c++", "clang++")] + [os.path.join(rocm, d, "bin", "clang++") for d in ("llvm", "lib/llvm")]
    cxx = next((c for c in found if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler"
    assert _run_program(tmp_path, cxx, []) == ACCEPTED


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def test_workspace_queries_accept_the_same_shapes(lib):
    """The entry points themselves (no launch, no device): a workspace query answers MTBT_EINVAL exactly outside its family's shapes."""
    walk = [(H, W) for H in HS for W in WS] + [(32768, 65535), (32768, 65536), (0, 64), (64, 0)]
    queries = {
        "dims": [lambda H, W: lib.mtbt_surface_distances_workspace_bytes(1, H, W), lambda H, W: lib.mtbt_distance_transform_workspace_bytes(1, H, W),
                 lambda H, W: lib.mtbt_seg_region_loss_workspace_bytes(1, H, W), lambda H, W: lib.mtbt_contours_workspace_bytes(1, H, W, 0),
                 lambda H, W: lib.mtbt_rle_workspace_bytes(1, H, W)],
        "components": [lambda H, W: lib.mtbt_components_workspace_bytes(1, H, W)],
    }
    for family, fns in queries.items():
        ok = {(H, W) for H, W, _ in ACCEPTED[family]}
        for i, fn in enumerate(fns):
            for H, W in walk:
                r = fn(H, W)
                assert (r >= 0) == ((H, W) in ok) and (r >= 0 or r == -1), (family, i, H, W, r)
    assert lib.mtbt_surface_distances_workspace_bytes(-1, 64, 64) == -1 and lib.mtbt_components_workspace_bytes(-1, 64, 64) == -1


# every name multitask_bonetumor_yolo_amd/__init__.py exported before planes.py existed
EXPORTED = (
    "ConvNeXtBiFPNYOLO", "ConvNeXtBiFPNYOLOv0", "ConvNeXtBiFPNYOLOv2", "DetectionConfusionMatrix", "DeviceMaskMeanAveragePrecision",
    "DeviceMeanAveragePrecision", "GraphedInference", "ImageClassificationMetrics", "InstanceMaskLoss", "LesionMetrics", "MeanAveragePrecision",
    "SegRegionLoss", "SegmentationMetrics", "SurfaceDistanceMetrics", "TaskAlignedDetLoss", "TaskAlignedSegLoss", "TrainStep", "ValidationStep",
    "affine_coefficients", "affine_forward", "affine_polygons", "affine_samples", "affine_samples_seg", "affine_yolo_labels", "augment_batch",
    "augment_polygons", "augment_samples", "augment_samples_seg", "augment_yolo_labels", "calibrate_synthetic_heads_", "clahe_batch", "clahe_clip",
    "coco_segm_results", "components_to_instances", "contour_polygons", "copy_paste_batch", "count_contour_vertices", "detect_fused",
    "detect_sliced", "distance_transform", "ema_decay_at", "fill_polygons", "filter_components", "init_synthetic_", "instance_mask_loss",
    "label_components", "labelme_shapes", "lesion_hits", "letterbox_geometry", "load_pretrained_heads", "load_train_state", "merge_tiles",
    "mosaic_batch", "mosaic_polygons", "mosaic_samples", "mosaic_samples_seg", "mosaic_yolo_labels", "multitask_loss", "photometric_lut",
    "postprocess", "preprocess", "rle_encode", "rle_from_string", "rle_to_string", "sample_affine", "sample_clahe", "sample_copy_paste",
    "sample_geometry", "sample_mosaic", "sample_photometric", "save_train_state", "seg_region_loss", "seg_to_frames", "signed_distance",
    "slice_batch", "slice_geometry", "strip_lightning_prefix", "surface_distances", "surface_metrics", "synthetic_images", "task_aligned_det_loss",
    "trace_contours", "vote_masks", "vote_tile_masks", "warp_batch", "yolo_seg_planes", "yolo_seg_polygons", "yolo_seg_rows",
)


def test_moved_names_stay_where_they_were():
    import multitask_bonetumor_yolo_amd as pkg
    from multitask_bonetumor_yolo_amd import planes, postprocess
    moved = ("unpack_masks", "pack_masks", "label_components", "filter_components", "components_to_instances", "distance_transform",
             "signed_distance", "fill_polygons", "yolo_seg_planes", "yolo_seg_polygons", "count_contour_vertices", "trace_contours",
             "contour_polygons", "yolo_seg_rows", "labelme_shapes", "rle_encode", "rle_to_string", "rle_from_string", "coco_segm_results",
             "COMPONENTS_MAX_DIM", "COMPONENTS_MAX_TABLE", "D2_NONE", "POLYGON_MAX_COORD")
    for name in moved:
        assert getattr(postprocess, name) is getattr(planes, name), name
    for name in EXPORTED:
        assert getattr(pkg, name) is not None, name
    assert pkg.planes is planes and pkg.label_components is planes.label_components and pkg.rle_encode is planes.rle_encode
    assert planes.plane_pitch(1) == 8 and planes.plane_pitch(64) == 8 and planes.plane_pitch(65) == 16 and planes.plane_pitch(16385) == 2056
