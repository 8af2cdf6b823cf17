"""Operators on bit-packed mask planes, on the device: the layout in one place (`plane_pitch`, `packed_planes`), packing and unpacking,
connected components, region measurements (hull, Feret diameters, moments), the exact distance transform, polygons in (`fill_polygons`)
and out (`trace_contours`), COCO run lengths.

A stack of planes is uint8 [n, H, pitch] with pitch = 8 * ceil(W / 64) bytes per row: 64 pixels per 8-byte word, pixel X is bit X & 7 of
byte X >> 3 (numpy.packbits(bitorder="little")), padding bits X >= W never count.  `postprocess.masks_to_frames`, `vote_masks`,
`vote_tile_masks` and `seg_to_frames` write such planes; `metrics` and `loss` read them.  csrc/bitplane.h is the same for the kernels.
Every name here is also importable from `postprocess`, where these operators first lived.  No CPU path.
"""
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L


def plane_pitch(W: int) -> int:
    """Bytes of a row of a packed plane of W pixels: whole 8-byte words of 64 pixels."""
    return 8 * ((int(W) + 63) // 64)


def _need_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: expected a CUDA/HIP tensor on an MI355X (no CPU path)")


def unpack_masks(packed: torch.Tensor, W0: int) -> torch.Tensor:
    """uint8 [K, H0, pitch] bit planes of `masks_to_frames` -> bool [K, H0, W0], on the tensor's device."""
    shifts = torch.arange(8, dtype=torch.uint8, device=packed.device)
    bits = (packed.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(packed.shape[0], packed.shape[1], packed.shape[2] * 8)[:, :, :W0].bool()


def pack_masks(planes: torch.Tensor, boxes: Optional[torch.Tensor] = None, plane_of: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense masks -> the bit-packed planes of `masks_to_frames` (`unpack_masks` is the inverse), on the device (`mtbt_pack_masks`).

    planes [n, H, W] bool, uint8 or float32 (bit = value > 0, NaN -> 0).  `plane_of` (int [n_out]): output j is made from source plane
    plane_of[j]; an index outside [0, n) gives a zero plane.  `boxes` (float32 [n_out, 4] xyxy pixels): output j keeps only
    x1 <= X < x2 and y1 <= Y < y2, the crop rule of `masks_to_frames`.  Together they build per-box instance ground truth from one mask
    per image and its box rows.  Returns uint8 [n_out, H, pitch], pitch = 8 * ceil(W / 64), padding bits zero.  `out=` takes a caller's
    contiguous uint8 [n_out, H, pitch] tensor (8-byte aligned); every byte of it is written, whatever it held.  Asynchronous."""
    lib = L.load()
    _need_cuda(planes, "pack_masks")
    if planes.dim() != 3 or planes.dtype not in (torch.bool, torch.uint8, torch.float32):
        raise ValueError("pack_masks: planes must be [n, H, W] bool, uint8 or float32")
    n, H, W = planes.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"pack_masks: planes of {H} x {W} pixels (1 <= H * W < 2^31)")
    dev = planes.device
    if planes.dtype == torch.bool:
        planes = planes.view(torch.uint8)
    if n and (planes.stride(2) != 1 or planes.stride(1) < W or planes.stride(0) < 0):
        planes = planes.contiguous()
    n_out = n
    if plane_of is not None:
        _need_cuda(plane_of, "pack_masks")
        plane_of = plane_of.reshape(-1).to(torch.int32).contiguous()
        n_out = plane_of.numel()
    if boxes is not None:
        _need_cuda(boxes, "pack_masks")
        boxes = boxes.to(torch.float32).contiguous()
        if boxes.dim() != 2 or boxes.shape[1] != 4 or (plane_of is not None and boxes.shape[0] != n_out) or (plane_of is None and boxes.shape[0] != n):
            raise ValueError(f"pack_masks: boxes must be [{n_out}, 4] xyxy, one row per output plane")
    pitch = plane_pitch(W)
    if out is None:
        out = torch.empty((n_out, H, pitch), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n_out, H, pitch) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"pack_masks: out must be a contiguous uint8 [{n_out}, {H}, {pitch}] tensor on {dev}")
    if n_out == 0:
        return out
    a = L.PackMasksArgs()
    a.src = planes.data_ptr() if n else None
    a.plane_of = plane_of.data_ptr() if plane_of is not None else None
    a.boxes = boxes.data_ptr() if boxes is not None else None
    a.out = out.data_ptr()
    a.plane_stride, a.row_stride = (planes.stride(0), planes.stride(1)) if n else (H * W, W)
    a.n_src, a.n_out, a.H, a.W, a.pitch, a.dtype = n, n_out, H, W, pitch, int(planes.dtype == torch.float32)
    with torch.cuda.device(dev):
        L.check(lib.mtbt_pack_masks(C.byref(a), L.stream(dev)), "mtbt_pack_masks")
    return out


# ---- connected components of packed planes ----------------------------------------------------------------------------------------
COMPONENTS_MAX_DIM = 16384       # H and W of mtbt_label_components
COMPONENTS_MAX_TABLE = 65536     # max_components


def packed_planes(what: str, packed: torch.Tensor, W: int, other: Optional[torch.Tensor] = None, max_dim: int = COMPONENTS_MAX_DIM, words=None):
    """The argument check of the operators that take a stack of packed planes (`other`: a second stack of the same shape) ->
    (n, H, pitch, packed and other made contiguous and 8-byte aligned).  Refusals carry the operator's name `what` in front.  `words`:
    the caller's own wording of the three refusals of the stacks themselves (packed's form; other's dtype or shape; other's device)."""
    for t in (packed,) + (() if other is None else (other,)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{what}: expected CUDA/HIP tensors on an MI355X (no CPU path)")
    if words is None:
        words = ("packed must be uint8 [n, H, pitch]",) + (f"other must be uint8 of packed's shape {tuple(packed.shape)}, on its device",) * 2
    if packed.dim() != 3 or packed.dtype != torch.uint8:
        raise ValueError(f"{what}: {words[0]}")
    if other is not None and (other.dtype != torch.uint8 or other.shape != packed.shape):
        raise ValueError(f"{what}: {words[1]}")
    if other is not None and other.device != packed.device:
        raise ValueError(f"{what}: {words[2]}")
    n, H, pitch = (int(v) for v in packed.shape)
    if not (1 <= H <= max_dim and 1 <= W <= max_dim):
        raise ValueError(f"{what}: planes of {H} x {W} pixels (1 <= H, W <= {max_dim})")
    if pitch != plane_pitch(W):
        raise ValueError(f"{what}: packed planes of width {W} are uint8 [n, H, {plane_pitch(W)}]")
    planes = []
    for t in (packed, other):
        if t is not None:
            t = t.contiguous()
            t = t if t.data_ptr() % 8 == 0 else t.clone()
        planes.append(t)
    return n, H, pitch, planes[0], planes[1]


def label_components(packed: torch.Tensor, W: int, *, connectivity: int = 4, max_components: int = 1024,
                     other: Optional[torch.Tensor] = None, want_labels: bool = True):
    """Connected components of n bit-packed planes, on the device (`mtbt_label_components`; definitions in include/mtbt_hip.h).

    packed: uint8 [n, H, pitch] with pitch = 8 * ceil(W / 64) (`pack_masks`, `masks_to_frames`); bits X >= W never count.
    `connectivity` 4 or 8.  The components of a plane are numbered 1 .. n_components in row-major order of their first pixel (the
    numbering of `scipy.ndimage.label`); 0 is background.  Returns a dict of device tensors: `labels` int32 [n, H, W] (None with
    want_labels=False), `n_components` int32 [n] (the true count), and for the ids 1 .. min(n_components, max_components), id i in
    row i - 1, `area` int32 [n, C], `boxes` float32 [n, C, 4] xyxy with exclusive maxima (usable as `pack_masks(boxes=)`), `first`
    int32 [n, C] (flat index of the first pixel) and, with a second stack `other` of the same shape, `inter` int32 [n, C] =
    popcount(component & other's plane) (None without).  Rows beyond n_components are zero.  `shape` = (H, W).  Asynchronous: no
    host synchronisation; the result is a pure function of the input."""
    W, connectivity, C_ = int(W), int(connectivity), int(max_components)
    n, H, pitch, planes, oth = packed_planes("label_components", packed, W, other)
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity 4 or 8, not {connectivity}")
    if not 1 <= C_ <= COMPONENTS_MAX_TABLE:
        raise ValueError(f"label_components: max_components {C_} is outside [1, {COMPONENTS_MAX_TABLE}]")
    dev = packed.device
    out = {"labels": torch.empty((n, H, W), dtype=torch.int32, device=dev) if want_labels else None,
           "n_components": torch.empty((n,), dtype=torch.int32, device=dev), "area": torch.empty((n, C_), dtype=torch.int32, device=dev),
           "first": torch.empty((n, C_), dtype=torch.int32, device=dev),
           "inter": torch.empty((n, C_), dtype=torch.int32, device=dev) if oth is not None else None, "shape": (H, W)}
    box = torch.empty((n, C_, 4), dtype=torch.int32, device=dev)
    if n == 0:
        out["boxes"] = box.float()
        return out
    lib = L.load()
    ws, ws_bytes = L.workspace(lib.mtbt_components_workspace_bytes, n, H, W, device=dev, what="mtbt_components_workspace_bytes")
    a = L.ComponentsArgs()
    a.packed, a.other, a.workspace, a.workspace_bytes = planes.data_ptr(), oth.data_ptr() if oth is not None else None, ws.data_ptr(), ws_bytes
    a.labels = out["labels"].data_ptr() if want_labels else None
    a.n_components, a.area, a.box, a.first = out["n_components"].data_ptr(), out["area"].data_ptr(), box.data_ptr(), out["first"].data_ptr()
    a.inter = out["inter"].data_ptr() if oth is not None else None
    a.n, a.H, a.W, a.pitch, a.connectivity, a.max_components = n, H, W, pitch, connectivity, C_
    with torch.cuda.device(dev):
        L.check(lib.mtbt_label_components(C.byref(a), L.stream(dev)), "mtbt_label_components")
    out["boxes"] = box.float()
    out["_keep"] = (planes, ws, ws_bytes)                     # what `mtbt_select_components` continues from
    return out


def filter_components(packed: torch.Tensor, W: int, *, min_area: int = 0, keep_largest: Optional[int] = None, connectivity: int = 4):
    """Remove components of n bit-packed planes, on the device (`mtbt_label_components` then `mtbt_select_components`).

    A component stays when its area is at least `min_area` and, with `keep_largest` = k > 0, it is among the k largest of its plane
    (equal areas: the lower id, i.e. the earlier first pixel); exact however many components a plane has.  Returns (packed uint8
    [n, H, pitch] with zero padding bits, n_kept int32 [n]).  Asynchronous."""
    W, min_area, k = int(W), int(min_area), int(keep_largest or 0)
    if not 0 <= min_area < 2 ** 32 or not 0 <= k < 2 ** 31:
        raise ValueError("filter_components: min_area and keep_largest must be >= 0 (and fit 32 bits)")
    rec = label_components(packed, W, connectivity=connectivity, max_components=1, want_labels=False)
    n, H, pitch = (int(v) for v in packed.shape)
    dev = packed.device
    out = torch.empty((n, H, pitch), dtype=torch.uint8, device=dev)
    n_kept = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return out, n_kept
    planes, ws, ws_bytes = rec["_keep"]
    a = L.SelectComponentsArgs()
    a.packed, a.workspace, a.workspace_bytes, a.out, a.n_kept = planes.data_ptr(), ws.data_ptr(), ws_bytes, out.data_ptr(), n_kept.data_ptr()
    a.n, a.H, a.W, a.pitch, a.min_area, a.keep_largest = n, H, W, pitch, min_area, k
    with torch.cuda.device(dev):
        L.check(L.load().mtbt_select_components(C.byref(a), L.stream(dev)), "mtbt_select_components")
    return out, n_kept


def components_to_instances(packed: torch.Tensor, W: int, *, max_instances: int = 100, min_area: int = 0, connectivity: int = 4):
    """The largest components of each of n bit-packed planes as instance planes: a semantic mask in the layout the instance consumers
    read (`det["masks_frame"][b]`, `DeviceMaskMeanAveragePrecision`, `SurfaceDistanceMetrics.update_packed`).

    Per plane the up to K = `max_instances` largest components of at least `min_area` pixels, largest first (equal areas: the earlier
    first pixel).  Returns a dict: `masks` uint8 [n, K, H, pitch] (masks[b] is [K, H, pitch]; the slots from counts[b] on are zero),
    `boxes` float32 [n, K, 4] xyxy, `areas` int32 [n, K], `counts` int32 [n].  `filter_components`, `label_components` and
    `pack_masks` with torch indexing between them; no host synchronisation."""
    K = int(max_instances)
    if not 1 <= K <= COMPONENTS_MAX_TABLE:
        raise ValueError(f"components_to_instances: max_instances {K} is outside [1, {COMPONENTS_MAX_TABLE}]")
    kept, counts = filter_components(packed, W, min_area=min_area, keep_largest=K, connectivity=connectivity)
    rec = label_components(kept, W, connectivity=connectivity, max_components=K)      # at most K components are left: the tables hold all
    n, H, pitch = (int(v) for v in kept.shape)
    areas, order = torch.sort(rec["area"], dim=1, descending=True, stable=True)
    slot = torch.arange(K, device=kept.device)[None, :]
    ids = torch.where(slot < counts[:, None], order + 1, -1).to(torch.int32)            # -1: no pixel carries it
    boxes = torch.gather(rec["boxes"], 1, order[:, :, None].expand(n, K, 4))
    masks = torch.empty((n, K, H, pitch), dtype=torch.uint8, device=kept.device)
    for b in range(n):
        pack_masks(rec["labels"][b][None] == ids[b][:, None, None], out=masks[b])
    return {"masks": masks, "boxes": boxes, "areas": areas, "counts": counts}


# ---- measurements of regions: sums, lattice hull, Feret diameters, minimum rectangle (THE MEASURE RULE: include/mtbt_hip.h) ----------
def measure_regions(packed: Optional[torch.Tensor], W: int, *, labels: Optional[torch.Tensor] = None, max_regions: int = 1024,
                    max_hull: int = 512) -> dict:
    """The exact integer measurements of regions, on the device (`mtbt_measure_regions`; THE MEASURE RULE is in include/mtbt_hip.h).

    Plane mode (labels=None): packed uint8 [n, H, pitch]; the one region of a plane is its set bits with X < W, connected or not
    (C = 1, `max_regions` is ignored): `det["masks_frame"][b]` and `seg_frame` as they are.  Label mode: labels int32 [n, H, W] (as
    `label_components` returns them; any label map will do), region i is {label == i} for 1 <= i <= C = max_regions; `packed` may
    then be None.  Returns a dict of device tensors, no read-back: `sums` int64 [n, C, 8] (area, perimeter, sum X, sum Y, sum X^2,
    sum X Y, sum Y^2, 0), `n_hull` int32 [n, C] (true), `hull` int32 [n, C, max_hull, 2] (x, y; the first min(n_hull, max_hull)
    vertices of the convex hull of the pixel squares, from the top-left one, clockwise on the screen; zero rows after them),
    `hull_area2` int64 [n, C], `caliper` int64 [n, C, 8] (d2, perp, w_num, w_len2, r_h, r_t, r_tmin, r_len2) and `caliper_at` int32
    [n, C, 8] (xa, ya, xb, yb, w_edge, w_vertex, r_edge, 0).  `shape` = (H, W).  An empty region is all zeros.  No measurement depends
    on `max_hull`.  `region_properties` turns the tables into lengths, areas and angles.  Asynchronous."""
    W, Vh = int(W), int(max_hull)
    if labels is None:
        n, H, pitch, planes, _ = packed_planes("measure_regions", packed, W)
        C_, dev = 1, packed.device
    else:
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
            raise RuntimeError("measure_regions: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if labels.dim() != 3 or labels.dtype != torch.int32 or int(labels.shape[2]) != W:
            raise ValueError(f"measure_regions: labels must be int32 [n, H, {W}]")
        n, H = int(labels.shape[0]), int(labels.shape[1])
        if not (1 <= H <= COMPONENTS_MAX_DIM and 1 <= W <= COMPONENTS_MAX_DIM):
            raise ValueError(f"measure_regions: maps of {H} x {W} pixels (1 <= H, W <= {COMPONENTS_MAX_DIM})")
        C_, dev, pitch, planes = int(max_regions), labels.device, plane_pitch(W), None
        labels = labels.contiguous()
        if not 1 <= C_ <= COMPONENTS_MAX_TABLE:
            raise ValueError(f"measure_regions: max_regions {C_} is outside [1, {COMPONENTS_MAX_TABLE}]")
    if Vh < 4 or Vh >= 2 ** 31:
        raise ValueError(f"measure_regions: max_hull {Vh} is below 4 (one pixel has four hull vertices)")
    out = {"sums": torch.empty((n, C_, 8), dtype=torch.int64, device=dev), "n_hull": torch.empty((n, C_), dtype=torch.int32, device=dev),
           "hull": torch.empty((n, C_, Vh, 2), dtype=torch.int32, device=dev), "hull_area2": torch.empty((n, C_), dtype=torch.int64, device=dev),
           "caliper": torch.empty((n, C_, 8), dtype=torch.int64, device=dev), "caliper_at": torch.empty((n, C_, 8), dtype=torch.int32, device=dev),
           "shape": (H, W)}
    if n == 0:
        return out
    lib = L.load()
    ws, ws_bytes = L.workspace(lib.mtbt_measure_workspace_bytes, n, H, W, C_, device=dev, what="mtbt_measure_workspace_bytes")
    a = L.MeasureArgs()
    a.packed, a.labels = planes.data_ptr() if planes is not None else None, labels.data_ptr() if labels is not None else None
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.sums, a.n_hull, a.hull, a.hull_area2 = out["sums"].data_ptr(), out["n_hull"].data_ptr(), out["hull"].data_ptr(), out["hull_area2"].data_ptr()
    a.caliper, a.caliper_at = out["caliper"].data_ptr(), out["caliper_at"].data_ptr()
    a.n, a.H, a.W, a.pitch, a.max_regions, a.max_hull = n, H, W, pitch, C_, Vh
    with torch.cuda.device(dev):
        L.check(lib.mtbt_measure_regions(C.byref(a), L.stream(dev)), "mtbt_measure_regions")
    return out


def measure_components(packed: torch.Tensor, W: int, *, connectivity: int = 4, max_components: int = 1024, max_hull: int = 512):
    """`label_components`, then `measure_regions` in label mode over its label map: the measurements of every connected component, id i
    in row i - 1.  Returns (the components dict, the measurements dict).  Asynchronous."""
    rec = label_components(packed, W, connectivity=connectivity, max_components=max_components)
    return rec, measure_regions(None, W, labels=rec["labels"], max_regions=max_components, max_hull=max_hull)


def region_properties(result: dict, *, spacing: float = 1.0) -> dict:
    """The tables of `measure_regions` as float64 numpy arrays of shape [n, C] (points [n, C, 2], `min_rect` [n, C, 4, 2]): reads the
    small tables back (synchronises) and finishes the floats on the host, as `surface_metrics` does.

    `area`, `perimeter` (pixel sides), `centroid` (sum X / A + 0.5, sum Y / A + 0.5: lattice coordinates), `mu20`, `mu02`, `mu11` (central
    second moments with the pixel's own 1/12), `orientation` = atan2(2 mu11, mu20 - mu02) / 2, `major_axis` and `minor_axis` = 4 sqrt of
    the eigenvalues, `eccentricity`, `equivalent_diameter` = sqrt(4 A / pi), `hull_area`, `solidity` = A / hull_area, `feret_max` with
    its end points `feret_a`, `feret_b`, `feret_perp` (the extent across it), `who_product` = feret_max * feret_perp, `feret_min` (the
    caliper width) and `min_rect` (the four corners of the minimum-area rectangle, in hull order) with `min_rect_area`; `n_hull`.
    `spacing` (length of a pixel side) scales lengths and points, its square areas and moments.  An empty region has 0 for sizes and
    NaN for ratios, angles and points; `min_rect` is also NaN where the rectangle's edge lies beyond the `max_hull` stored vertices
    (`min_rect_area` does not need them)."""
    sp = float(spacing)
    s = result["sums"].cpu().numpy().astype(np.float64)
    cal = result["caliper"].cpu().numpy()
    at = result["caliper_at"].cpu().numpy()
    hull = result["hull"].cpu().numpy().astype(np.float64)
    n_hull = result["n_hull"].cpu().numpy()
    a2 = result["hull_area2"].cpu().numpy().astype(np.float64)
    A = s[..., 0]
    nz = A > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        mx, my = s[..., 2] / A, s[..., 3] / A
        mu20, mu02, mu11 = s[..., 4] / A - mx * mx + 1.0 / 12.0, s[..., 6] / A - my * my + 1.0 / 12.0, s[..., 5] / A - mx * my
        half, root = (mu20 + mu02) / 2.0, np.sqrt(((mu20 - mu02) / 2.0) ** 2 + mu11 ** 2)
        l1, l2 = half + root, np.maximum(half - root, 0.0)
        d2, perp = cal[..., 0].astype(np.float64), cal[..., 1].astype(np.float64)
        fmax = np.sqrt(d2)
        fperp = perp / fmax
        fmin = cal[..., 2].astype(np.float64) / np.sqrt(cal[..., 3].astype(np.float64))
        r_h, r_t, r_tmin, r_len2 = (cal[..., k].astype(np.float64) for k in (4, 5, 6, 7))
        solidity = A / (a2 / 2.0)
        ecc = np.sqrt(1.0 - l2 / l1)
        # the rectangle on edge r_edge = p -> p + e: along e from tmin to tmax (in units of |e|^2), across it from 0 to h on the hull's side
        Vh = hull.shape[2]
        i0 = at[..., 6].astype(np.int64)
        i1 = (i0 + 1) % np.maximum(n_hull, 1)
        known = nz & (i0 < Vh) & (i1 < Vh)                                                # both ends of the edge are among the stored vertices
        row = lambda i: np.take_along_axis(hull, np.broadcast_to(np.clip(i, 0, Vh - 1)[..., None, None], i.shape + (1, 2)), axis=2)[..., 0, :]
        p0, p1 = row(i0), row(i1)
        e = p1 - p0
        nrm = np.stack([-e[..., 1], e[..., 0]], axis=-1)                                  # e turned clockwise on the screen: towards the hull
        lo, hi, hh = (r_tmin / r_len2)[..., None], ((r_tmin + r_t) / r_len2)[..., None], (r_h / r_len2)[..., None]
        rect = np.stack([p0 + lo * e, p0 + hi * e, p0 + hi * e + hh * nrm, p0 + lo * e + hh * nrm], axis=-2)
        rect_area = r_h * r_t / r_len2
    rect = np.where(known[..., None, None], rect, np.nan)
    nan = lambda v: np.where(nz, v, np.nan)
    zero = lambda v: np.where(nz, v, 0.0)
    pts = lambda k: np.where(nz[..., None], at[..., k:k + 2].astype(np.float64), np.nan) * sp
    return {"area": A * sp * sp, "perimeter": s[..., 1] * sp, "centroid": np.stack([nan(mx + 0.5), nan(my + 0.5)], axis=-1) * sp,
            "mu20": nan(mu20) * sp * sp, "mu02": nan(mu02) * sp * sp, "mu11": nan(mu11) * sp * sp,
            "orientation": nan(0.5 * np.arctan2(2.0 * mu11, mu20 - mu02)), "major_axis": zero(4.0 * np.sqrt(l1)) * sp,
            "minor_axis": zero(4.0 * np.sqrt(l2)) * sp, "eccentricity": nan(ecc), "equivalent_diameter": np.sqrt(4.0 * A / np.pi) * sp,
            "hull_area": a2 / 2.0 * sp * sp, "solidity": nan(solidity), "feret_max": zero(fmax) * sp, "feret_a": pts(0), "feret_b": pts(2),
            "feret_perp": zero(fperp) * sp, "who_product": zero(fmax * fperp) * sp * sp, "feret_min": zero(fmin) * sp,
            "min_rect": rect * sp, "min_rect_area": zero(rect_area) * sp * sp, "n_hull": n_hull}


def measure_detections(out: dict, *, spacing: float = 1.0, frames=None, max_hull: int = 512):
    """The measurements of the kept instance masks of a batch: a list, one `region_properties` dict per image, over the first
    counts[b] planes of `out["masks_frame"][b]` (plane mode; arrays of shape [counts[b], 1]).

    `out`: a `detect_and_segment(..., frames=...)` result (or `detect_fused` / `detect_sliced`); `frames`: the [(H0, W0, scale)] it was
    made with (or `out["frames"]`): the packed planes do not carry their width.  Synchronises."""
    frames = out.get("frames") if frames is None else frames
    B = len(out["masks_frame"])
    if frames is None or len(frames) != B:
        raise ValueError(f"measure_detections: {B} images need as many frames (H0, W0, scale)")
    n_kept = out["counts"].cpu().numpy()
    return [region_properties(measure_regions(out["masks_frame"][b][:int(n_kept[b])], int(frames[b][1]), max_hull=max_hull), spacing=spacing)
            for b in range(B)]


# ---- exact Euclidean distance transform of bit-packed planes (include/mtbt_hip.h `mtbt_distance_transform`) -------------------------
D2_NONE = 0xFFFFFFFF             # the word of a map whose plane holds no target pixel at all


def distance_transform(packed: torch.Tensor, W: int, *, to: str = "set"):
    """Squared Euclidean distance maps of n bit-packed planes, exact integers, on the device (`mtbt_distance_transform`).

    packed: uint8 [n, H, pitch] with pitch = 8 * ceil(W / 64) (`pack_masks`, `masks_to_frames`); bits X >= W never count.
    `to="set"`: uint32 [n, H, W], at every pixel the minimum of dy^2 + dx^2 over the SET pixels of its plane (0 on a set pixel;
    `scipy.ndimage.distance_transform_edt(~m) ** 2`).  `to="unset"`: the same over the unset pixels inside the image
    (`distance_transform_edt(m) ** 2`).  `to="both"`: the pair (to set, to unset) from one call.  A map whose plane holds no such
    pixel (an empty plane; a full one) is `D2_NONE` = 0xFFFFFFFF everywhere.  Asynchronous: no host synchronisation."""
    if to not in ("set", "unset", "both"):
        raise ValueError(f"distance_transform: to = 'set', 'unset' or 'both', not {to!r}")
    W = int(W)
    n, H, pitch, planes, _ = packed_planes("distance_transform", packed, W)
    dev = packed.device
    d_set = torch.empty((n, H, W), dtype=torch.uint32, device=dev) if to != "unset" else None
    d_unset = torch.empty((n, H, W), dtype=torch.uint32, device=dev) if to != "set" else None
    if n:
        lib = L.load()
        ws, ws_bytes = L.workspace(lib.mtbt_distance_transform_workspace_bytes, n, H, W, device=dev, what="mtbt_distance_transform_workspace_bytes")
        a = L.DistanceTransformArgs()
        a.packed, a.workspace, a.workspace_bytes = planes.data_ptr(), ws.data_ptr(), ws_bytes
        a.d2_set = d_set.data_ptr() if d_set is not None else None
        a.d2_unset = d_unset.data_ptr() if d_unset is not None else None
        a.n, a.H, a.W, a.pitch = n, H, W, pitch
        with torch.cuda.device(dev):
            L.check(lib.mtbt_distance_transform(C.byref(a), L.stream(dev)), "mtbt_distance_transform")
    return (d_set, d_unset) if to == "both" else (d_set if to == "set" else d_unset)


def signed_distance(packed: torch.Tensor, W: int) -> torch.Tensor:
    """The signed distance map of Kervadec et al.'s boundary loss (`one_hot2dist`), fp32 [n, H, W]: +sqrt(d2 to set) on an unset pixel,
    -(sqrt(d2 to unset) - 1) on a set pixel, 0 where the map it needs has no target (an empty and a full plane are zero everywhere).
    `distance_transform(to="both")` and torch ops on its maps (sqrt in float64: above 2^24 a float32 no longer holds d2)."""
    d_set, d_unset = distance_transform(packed, W, to="both")
    t = unpack_masks(packed, int(W))
    d2 = torch.where(t, d_unset.to(torch.int64), d_set.to(torch.int64))
    d = d2.to(torch.float64).sqrt().to(torch.float32)
    phi = torch.where(t, -(d - 1.0), d)
    return torch.where(d2 == D2_NONE, torch.zeros_like(phi), phi)


# ---- polygons -> bit-packed planes (the project's own fill rule: include/mtbt_hip.h `mtbt_fill_polygons`) ---------------------------
POLYGON_MAX_COORD = 32768.0      # |v| in pixels: 16 v fits int32 with room, and stays inside the kernel's clamp


def _polygons_of(entry, who: str):
    """One entry of `fill_polygons(planes)` -> its list of float64 [n_i, 2] arrays: an [n, 2] array-like is one polygon, a sequence of
    them their union."""
    as_np = lambda v: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    if isinstance(entry, (torch.Tensor, np.ndarray)) and getattr(entry, "dtype", None) != object:
        a = as_np(entry)
        if a.ndim == 2 and a.shape[1] == 2:
            return [a]
        if a.ndim == 3 and a.shape[2] == 2:
            return list(a)
        if a.size == 0:
            return []
        raise ValueError(f"{who}: a polygon must be an [n, 2] array of pixel coordinates, not {tuple(a.shape)}")
    items = list(entry)
    if items and (items[0].dim() if isinstance(items[0], torch.Tensor) else np.ndim(items[0])) == 1:   # a list of (x, y) pairs
        items = [items]
    polys = []
    for it in items:
        a = as_np(it)
        if a.size == 0:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"{who}: a polygon must be an [n, 2] array of pixel coordinates, not {tuple(a.shape)}")
        polys.append(a)
    return polys


def fill_polygons(planes: Sequence, H: int, W: int, *, clip=None, out: Optional[torch.Tensor] = None, records: bool = False, device=None):
    """Rasterise polygons into bit-packed planes on the device (`mtbt_fill_polygons`; the fill rule is in include/mtbt_hip.h: vertices
    in 1/16 pixel, pixel centres, even-odd per polygon, a plane the union of its polygons).

    `planes` has one entry per output plane: an [n_i, 2] array-like of pixel coordinates (one polygon), or a sequence of such arrays
    (their union; an empty sequence is an empty plane).  A polygon of fewer than 3 vertices fills nothing.  `clip`: an optional int
    [n, 4] of half-open pixel rectangles (x0, y0, x1, y1), one per plane (a mosaic tile).  Coordinates must be finite with
    |v| <= 32768 (ValueError).  They are quantised on the host, q = rint(float32(v) * 16), packed with the offset tables and the
    rectangles into one buffer that goes up in one asynchronous copy, and one call fills every plane.  Returns uint8 [n, H, pitch],
    pitch = 8 * ceil(W / 64), padding bits zero; with records=True also `area` int32 [n] and `boxes` float32 [n, 4] xyxy with
    exclusive maxima (zeros for an empty plane), as `label_components` returns them.  `out=` as in `pack_masks`.  Asynchronous; there
    is no CPU path."""
    lib = L.load()
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"fill_polygons: planes of {H} x {W} pixels (1 <= H * W < 2^31)")
    polys_of = [_polygons_of(e, "fill_polygons") for e in planes]
    n = len(polys_of)
    flat = [p for ps in polys_of for p in ps]
    verts = np.concatenate(flat, axis=0) if flat else np.zeros((0, 2), dtype=np.float64)
    if verts.size and not (np.isfinite(verts).all() and np.abs(verts).max() <= POLYGON_MAX_COORD):
        raise ValueError(f"fill_polygons: coordinates must be finite and within +-{int(POLYGON_MAX_COORD)} pixels")
    n_polys, n_vertices = len(flat), verts.shape[0]
    if n_vertices >= 2 ** 30:
        raise ValueError("fill_polygons: too many vertices")
    rects = None
    if clip is not None:
        rects = np.asarray(clip.cpu() if isinstance(clip, torch.Tensor) else clip)
        if rects.dtype.kind not in "iu" and rects.size:
            raise ValueError("fill_polygons: clip must be integer pixel rectangles")
        rects = rects.reshape(-1, 4) if rects.size or n == 0 else rects
        if rects.shape != (n, 4):
            raise ValueError(f"fill_polygons: clip must be [{n}, 4] (x0, y0, x1, y1), one row per plane")
        rects = np.clip(rects.astype(np.int64), -2 ** 31, 2 ** 31 - 1)
    dev = torch.device(device) if device is not None else (out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
    if dev.type != "cuda":
        raise RuntimeError("fill_polygons: expected a CUDA/HIP device (an MI355X; no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    pitch = plane_pitch(W)
    if out is None:
        out = torch.empty((n, H, pitch), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, H, pitch) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"fill_polygons: out must be a contiguous uint8 [{n}, {H}, {pitch}] tensor on {dev}")
    area = torch.empty((n,), dtype=torch.int32, device=dev) if records else None
    box = torch.empty((n, 4), dtype=torch.int32, device=dev) if records else None
    if n:
        # one host buffer: vertices | polygon offsets | plane offsets | clip rectangles, all int32
        o_poly, o_plane, o_clip = 2 * n_vertices, 2 * n_vertices + n_polys + 1, 2 * n_vertices + n_polys + 1 + n + 1
        host = torch.empty(o_clip + (4 * n if rects is not None else 0), dtype=torch.int32).pin_memory()
        h = host.numpy()
        h[:o_poly] = np.rint(verts.astype(np.float32) * np.float32(16.0)).astype(np.int32).reshape(-1)
        h[o_poly] = 0
        np.cumsum([p.shape[0] for p in flat], dtype=np.int32, out=h[o_poly + 1:o_plane])
        h[o_plane] = 0
        np.cumsum([len(ps) for ps in polys_of], dtype=np.int32, out=h[o_plane + 1:o_clip])
        if rects is not None:
            h[o_clip:] = rects.reshape(-1)
        buf = host.to(dev, non_blocking=True)
        a = L.FillPolygonsArgs()
        base = buf.data_ptr()
        a.vertices, a.poly_offsets, a.plane_offsets = base, base + 4 * o_poly, base + 4 * o_plane
        a.clip = base + 4 * o_clip if rects is not None else None
        a.out, a.area, a.box = out.data_ptr(), area.data_ptr() if records else None, box.data_ptr() if records else None
        a.n, a.n_polys, a.n_vertices, a.H, a.W, a.pitch = n, n_polys, n_vertices, H, W, pitch
        with torch.cuda.device(dev):
            L.check(lib.mtbt_fill_polygons(C.byref(a), L.stream(dev)), "mtbt_fill_polygons")   # buf is freed in stream order, after the launch
    return (out, area, box.float()) if records else out


def yolo_seg_planes(rows: Sequence[Sequence[float]], H0: int, W0: int, device=None):
    """YOLO-seg label rows (cls, x1, y1, x2, y2, ... normalised to the ORIGINAL image) -> (packed uint8 [G, H0, pitch], labels int64
    [G]) on the device: one plane per row in the image's own pixels, vertices at (x * W0, y * H0), filled by `fill_polygons`.  Rows of
    fewer than 3 points are skipped.  The per-image ground truth `DeviceMaskMeanAveragePrecision.update_batched` and
    `SurfaceDistanceMetrics.update_packed` take."""
    polys, labels = yolo_seg_polygons(rows, H0, W0)
    packed = fill_polygons(polys, H0, W0, device=device)
    labels = torch.tensor(labels, dtype=torch.int64)
    return packed, (labels.pin_memory().to(packed.device, non_blocking=True) if labels.numel() else labels.to(packed.device))


def yolo_seg_polygons(rows: Sequence[Sequence[float]], H0: int, W0: int):
    """The row parser of `yolo_seg_planes`, on the host: YOLO-seg rows -> (list of float64 [k, 2] polygons in the image's pixels,
    list of int classes).  Rows of fewer than 3 points are skipped."""
    polys, labels = [], []
    for r in rows:
        pts = [float(v) for v in r[1:]]
        k = len(pts) // 2
        if k < 3:
            continue
        v = np.asarray(pts[:2 * k], dtype=np.float64).reshape(k, 2)
        polys.append(v * np.asarray([float(W0), float(H0)]))
        labels.append(int(r[0]))
    return polys, labels


# ---- bit-packed planes -> polygons (THE CONTOUR RULE: include/mtbt_hip.h `mtbt_trace_contours`) -------------------------------------
def _count_contour_vertices(lib, planes, n, H, W, pitch, connectivity, dev):
    n_vertices = torch.empty((n,), dtype=torch.int32, device=dev)
    a = L.ContoursArgs()
    a.packed, a.n_vertices = planes.data_ptr(), n_vertices.data_ptr()
    a.n, a.H, a.W, a.pitch, a.connectivity = n, H, W, pitch, connectivity
    with torch.cuda.device(dev):
        L.check(lib.mtbt_trace_contours(C.byref(a), L.stream(dev)), "mtbt_trace_contours")
    return n_vertices


def count_contour_vertices(packed: torch.Tensor, W: int) -> torch.Tensor:
    """int32 [n]: the number of contour vertices of every plane (the count-only call of `mtbt_trace_contours`: one pass over 2 x 2
    pixel patterns, the same for both connectivities).  Asynchronous."""
    W = int(W)
    n, H, pitch, planes, _ = packed_planes("count_contour_vertices", packed, W)
    if n == 0:
        return torch.empty((0,), dtype=torch.int32, device=packed.device)
    return _count_contour_vertices(L.load(), planes, n, H, W, pitch, 4, packed.device)


def trace_contours(packed: torch.Tensor, W: int, *, connectivity: int = 4, max_contours: int = 1024, max_vertices: Optional[int] = None,
                   labels: Optional[torch.Tensor] = None):
    """The boundary polygons of n bit-packed planes, on the device (`mtbt_trace_contours`; THE CONTOUR RULE is in include/mtbt_hip.h).

    packed: uint8 [n, H, pitch] with pitch = 8 * ceil(W / 64) (`pack_masks`, `masks_to_frames`, `seg_to_frames`); bits X >= W never
    count.  A contour runs along pixel edges with the set pixels on its right; its vertices are lattice points (x, y), 0 <= x <= W,
    0 <= y <= H, the corners only.  At a vertex where two diagonal pixels meet, `connectivity` 4 keeps them apart and 8 joins them:
    the outer contours are then exactly the components of `label_components(connectivity=same)`, in id order.  Filling every contour
    with `fill_polygons` and XOR-ing the fills gives the plane back.  Returns a dict of device tensors:
      `n_vertices` int32 [n] (true), `n_contours` int32 [n] (true, or -1 for a plane with more than `max_vertices` vertices: its
      tables are then zero), `vertices` int32 [n, V, 2] (x, y; the contours back to back in order of their start),
      and for the first min(n_contours, max_contours) contours `offset`, `count`, `start` int32 [n, C] (start = y * (W + 1) + x of the
      first vertex, the top-left corner of the contour's first pixel row), `area2` int64 [n, C] (twice the signed area: > 0 outer,
      < 0 hole), `boxes` float32 [n, C, 4] xyxy over the vertices (for an outer contour the pixel box with exclusive maxima, as
      `label_components` returns it), `hole` bool [n, C];
      `component` int32 [n, C] when `labels` = label_components(..., connectivity=same)["labels"] is given: labels[y, x] of the pixel
      under the start edge, i.e. the component an outer contour bounds or a hole lies in (None otherwise; 0 in unused rows).
    `shape` = (H, W).  With max_vertices=None the vertices are counted first (`count_contour_vertices`), the largest count is read
    back and `vertices` is allocated exactly: ONE host synchronisation.  An explicit `max_vertices` never synchronises."""
    W, connectivity, C_ = int(W), int(connectivity), int(max_contours)
    n, H, pitch, planes, _ = packed_planes("trace_contours", packed, W)
    if connectivity not in (4, 8):
        raise ValueError(f"trace_contours: connectivity 4 or 8, not {connectivity}")
    if not 1 <= C_ <= COMPONENTS_MAX_TABLE:
        raise ValueError(f"trace_contours: max_contours {C_} is outside [1, {COMPONENTS_MAX_TABLE}]")
    if max_vertices is not None and not 0 <= int(max_vertices) < 2 ** 31:
        raise ValueError("trace_contours: max_vertices must be >= 0 (and fit 32 bits)")
    dev = packed.device
    if labels is not None and (not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (n, H, W) or labels.device != dev):
        raise ValueError(f"trace_contours: labels must be the [{n}, {H}, {W}] label map of label_components, on the planes' device")
    lib = L.load() if n else None
    if max_vertices is None:
        V = int(_count_contour_vertices(lib, planes, n, H, W, pitch, connectivity, dev).max()) if n else 0   # the host synchronisation
    else:
        V = int(max_vertices)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = {"n_vertices": i32(n), "n_contours": i32(n), "vertices": i32(n, V, 2), "offset": i32(n, C_), "count": i32(n, C_),
           "area2": torch.empty((n, C_), dtype=torch.int64, device=dev), "start": i32(n, C_), "shape": (H, W), "component": None}
    box = i32(n, C_, 4)
    if n:
        ws, ws_bytes = L.workspace(lib.mtbt_contours_workspace_bytes, n, H, W, V, device=dev, what="mtbt_contours_workspace_bytes")
        a = L.ContoursArgs()
        a.packed, a.workspace, a.workspace_bytes = planes.data_ptr(), ws.data_ptr(), ws_bytes
        a.n_vertices, a.n_contours, a.vertices = out["n_vertices"].data_ptr(), out["n_contours"].data_ptr(), out["vertices"].data_ptr()
        a.vertices = a.vertices or ws.data_ptr()               # V = 0: an empty tensor has no address; nothing is stored through it
        a.offset, a.count, a.area2, a.box, a.start = (out["offset"].data_ptr(), out["count"].data_ptr(), out["area2"].data_ptr(),
                                                      box.data_ptr(), out["start"].data_ptr())
        a.n, a.H, a.W, a.pitch, a.connectivity, a.max_contours, a.max_vertices = n, H, W, pitch, connectivity, C_, V
        with torch.cuda.device(dev):
            L.check(lib.mtbt_trace_contours(C.byref(a), L.stream(dev)), "mtbt_trace_contours")
    out["boxes"] = box.float()
    out["hole"] = out["area2"] < 0
    if labels is not None:
        used = out["count"] > 0
        sy, sx = torch.div(out["start"], W + 1, rounding_mode="floor"), out["start"] % (W + 1)
        flat = (sy.long() * W + sx.long()).clamp_(0, H * W - 1)                        # the pixel under the start edge is (x, y) itself
        out["component"] = torch.where(used, torch.gather(labels.reshape(n, H * W), 1, flat).to(torch.int32), torch.zeros_like(out["start"]))
    return out


def contour_polygons(result: dict, plane: int, holes: bool = False):
    """The polygons of one plane of a `trace_contours` result as a list of int32 [k, 2] numpy arrays (x, y), in contour order; the
    holes only with holes=True.  Reads the small tables and the plane's vertices back: synchronises.  A plane that did not fit
    `max_vertices` (n_contours = -1) or has more contours than `max_contours` raises ValueError."""
    plane = int(plane)
    nc, nv = int(result["n_contours"][plane]), int(result["n_vertices"][plane])
    C_ = int(result["offset"].shape[1])
    if nc < 0:
        raise ValueError(f"contour_polygons: plane {plane} has {nv} vertices, more than max_vertices = {int(result['vertices'].shape[1])}")
    if nc > C_:
        raise ValueError(f"contour_polygons: plane {plane} has {nc} contours, more than max_contours = {C_}")
    verts = result["vertices"][plane, :nv].cpu().numpy()
    off, cnt, hole = (result[k][plane, :nc].cpu().numpy() for k in ("offset", "count", "hole"))
    return [verts[o:o + c].astype(np.int32) for o, c, h in zip(off, cnt, hole) if holes or not h]


def yolo_seg_rows(result: dict, labels, W0: int, H0: int):
    """YOLO-seg label rows of a `trace_contours` result over planes of an image of W0 x H0 pixels: one row `[cls, x1, y1, x2, y2, ...]`
    per OUTER contour, coordinates normalised by W0 and H0, cls = labels[plane] (a sequence or tensor of one class per plane).  What
    `yolo_seg_planes` reads.  HOLES ARE OMITTED: the format cannot carry them, so a plane with holes comes back filled.  Synchronises."""
    labels = labels.tolist() if isinstance(labels, (torch.Tensor, np.ndarray)) else list(labels)
    n = int(result["n_contours"].shape[0])
    if len(labels) != n:
        raise ValueError(f"yolo_seg_rows: {len(labels)} labels for {n} planes")
    scale = np.asarray([float(W0), float(H0)])
    rows = []
    for b in range(n):
        for poly in contour_polygons(result, b):
            rows.append([int(labels[b])] + (poly.astype(np.float64) / scale).reshape(-1).tolist())
    return rows


def labelme_shapes(result: dict, plane: int, label: str):
    """The `shapes` list of a LabelMe file for one plane of a `trace_contours` result: one {"label", "points": [[x, y], ...],
    "shape_type": "polygon"} per OUTER contour (plus LabelMe's empty "group_id" and "flags").  HOLES ARE OMITTED: a LabelMe polygon
    cannot carry them.  Synchronises."""
    return [{"label": str(label), "points": poly.astype(np.float64).tolist(), "group_id": None, "shape_type": "polygon", "flags": {}}
            for poly in contour_polygons(result, plane)]


# ---- bit-packed planes -> COCO run lengths (THE RUN RULE: include/mtbt_hip.h `mtbt_rle_encode`) ------------------------------------
def rle_encode(packed: torch.Tensor, W: int, max_runs: Optional[int] = None):
    """The uncompressed COCO run lengths of n bit-packed planes, on the device (`mtbt_rle_encode`): the pixels read column-major
    (index x * H + y), runs alternating from a run of unset pixels (0 when pixel (0, 0) is set); their sum is H * W.

    Returns (`counts` int32 [n, R], `n_runs` int32 [n], the true number of runs).  Row b of `counts` holds its first
    min(n_runs[b], R) runs (every run is at most H * W < 2^31); the words beyond are unspecified.  With max_runs=None the runs are
    counted first, the largest count is read back and R is exact: ONE host synchronisation.  An explicit `max_runs` never
    synchronises; a plane with n_runs > R is cut."""
    W = int(W)
    n, H, pitch, planes, _ = packed_planes("rle_encode", packed, W)
    if max_runs is not None and not 0 <= int(max_runs) < 2 ** 31:
        raise ValueError("rle_encode: max_runs must be >= 0 (and fit 32 bits)")
    dev = packed.device
    n_runs = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        return torch.empty((0, int(max_runs or 0)), dtype=torch.int32, device=dev), n_runs
    lib = L.load()
    ws, ws_bytes = L.workspace(lib.mtbt_rle_workspace_bytes, n, H, W, device=dev, what="mtbt_rle_workspace_bytes")
    a = L.RleArgs()
    a.packed, a.workspace, a.workspace_bytes, a.n_runs = planes.data_ptr(), ws.data_ptr(), ws_bytes, n_runs.data_ptr()
    a.n, a.H, a.W, a.pitch = n, H, W, pitch
    with torch.cuda.device(dev):
        if max_runs is None:
            L.check(lib.mtbt_rle_encode(C.byref(a), L.stream(dev)), "mtbt_rle_encode")
            R = int(n_runs.max())                               # the host synchronisation
        else:
            R = int(max_runs)
        counts = torch.empty((n, R), dtype=torch.int32, device=dev)
        if R > 0 or max_runs is not None:
            a.counts, a.max_runs = (counts.data_ptr() if R > 0 else None), R
            L.check(lib.mtbt_rle_encode(C.byref(a), L.stream(dev)), "mtbt_rle_encode")
    return counts, n_runs


def rle_to_string(counts) -> str:
    """A run-length list as the compressed `counts` string of a COCO RLE (the pycocotools scheme): x[i] -= x[i - 2] for i > 2, every
    value in 5-bit groups, least significant first, 0x20 the continuation bit, bit 0x10 of the last group the sign, each group + 48
    as ASCII."""
    counts = [int(c) for c in counts]
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            out.append(chr((c | 0x20 if more else c) + 48))
    return "".join(out)


def rle_from_string(s: str):
    """The inverse of `rle_to_string`: the list of run lengths."""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def coco_segm_results(out: dict, image_ids, category_ids=None, frames=None):
    """The instance results of a batch as the list a COCO `segm` results file holds: for every kept detection
    {"image_id", "category_id", "score", "bbox": [x, y, w, h], "segmentation": {"size": [H0, W0], "counts": str}}.

    `out`: a `detect_and_segment(..., frames=...)` result (or `detect_fused` / `detect_sliced`): `masks_frame` (bit-packed planes per
    image), `boxes_frame`, `scores`, `labels`, `counts`.  `frames`: the [(H0, W0, scale)] the result was made with (or `out["frames"]`):
    the packed planes do not carry their width.  `image_ids`: one id per image.  `category_ids`: a sequence or dict from the label to the
    dataset's category id (None: the label itself).  The masks are run-length encoded on the device (`rle_encode`), only the runs come
    to the host; the strings are the pycocotools compression (`rle_to_string`).  Synchronises."""
    frames = out.get("frames") if frames is None else frames
    B = len(out["masks_frame"])
    if frames is None or len(frames) != B or len(image_ids) != B:
        raise ValueError(f"coco_segm_results: {B} images need as many frames (H0, W0, scale) and image ids")
    n_kept, scores, labels, boxes = (out[k].cpu().numpy() for k in ("counts", "scores", "labels", "boxes_frame"))
    results = []
    for b in range(B):
        H0, W0, k = int(frames[b][0]), int(frames[b][1]), int(n_kept[b])
        if k == 0:
            continue
        runs, n_runs = rle_encode(out["masks_frame"][b][:k], W0)
        runs, n_runs = runs.cpu().numpy(), n_runs.cpu().numpy()
        for j in range(k):
            lab = int(labels[b, j])
            x1, y1, x2, y2 = (float(v) for v in boxes[b, j])
            results.append({"image_id": image_ids[b], "category_id": lab if category_ids is None else category_ids[lab], "score": float(scores[b, j]),
                            "bbox": [x1, y1, x2 - x1, y2 - y1],
                            "segmentation": {"size": [H0, W0], "counts": rle_to_string(runs[j, :n_runs[j]].tolist())}})
    return results
