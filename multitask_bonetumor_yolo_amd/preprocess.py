"""Input pipeline of a batch on the device: what `BTXRDDataset.__getitem__` + `collate_fn`
(`/root/reference/src/dataset_btxrdv2.py:109-166`, `:168-245`, `:261-284`) do per sample on the CPU with cv2.

`letterbox_batch` is the image work (one HIP launch per <= 32 images, no CPU path); `transform_yolo_labels` and
`collate_boxes` are the label arithmetic, which is a handful of Python-float operations per box and stays on the host
exactly as the reference writes it.

Training augmentation (`augment_batch` and the functions after it) is NOT in the reference, whose dataset class augments
nothing: scale / aspect jitter, shift / crop, the eight dihedral orientations and an intensity table are this project's own
definition (include/mtbt_hip.h `mtbt_augment_batch`).  The image work is the letterbox's launch with the sampling place
chosen by the caller; the parameters are drawn and the labels moved on the host.

The four-image mosaic (`mosaic_batch` and the functions after it, include/mtbt_hip.h `mtbt_mosaic_batch`) is the same arithmetic
with the source picked per canvas region: a centre cuts the canvas into four rectangles, each showing its own image under its own
geometry row; with the centre at (S, S) a canvas is the plain augmentation of its first tile.

`warp_batch` (include/mtbt_hip.h `mtbt_warp_batch`, and the `affine_*` functions after it) turns and shears: an affine map per canvas in
fixed point, 2 x 2 taps, a kernel of its own because a rotated canvas row is neither a row nor a column of the source.  Its labels are
moved by the exact inverse of the integer map the pixels use; polygon labels stay tight under rotation, box labels grow.

`clahe_batch` (include/mtbt_hip.h `mtbt_clahe_batch`) equalises the raw uint8 images tile-wise at their own resolution before any of
the above: the project's own integer rule, modelled on cv2's CLAHE, which the reference does not use either.

`copy_paste_batch` (include/mtbt_hip.h `mtbt_copy_paste`) comes after all of them: it lays instances of other canvases of the batch, cut out
by their bit-packed planes, on a canvas -- pixels, planes and label rows together, exact copies, nothing resampled.  `sample_copy_paste` draws
its table from the host-side label rows; `copy_paste=dict(...)` of the `*_samples_seg` functions runs both.
"""
import ctypes as C
import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .planes import fill_polygons, plane_pitch, unpack_masks


def _descriptors(images, masks, who: str):
    """Validate raw images / masks and describe them for the library.  Returns (descs, tensors to keep alive, device)."""
    B = len(images)
    if B == 0:
        raise ValueError(f"{who}: empty batch")
    descs = (L.RawImage * B)()
    keep = []
    for i, im in enumerate(images):
        if not im.is_cuda:
            raise RuntimeError(f"{who}: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"{who}: images must be uint8 [H, W, 3] (BGR, as cv2.imread returns them)")
        if im.stride(2) != 1 or im.stride(1) != 3:
            im = im.contiguous()
        keep.append(im)
        d = descs[i]
        d.bgr, d.height, d.width, d.row_stride = im.data_ptr(), im.shape[0], im.shape[1], im.stride(0)
        mk = masks[i] if masks is not None else None
        if mk is not None:
            if mk.dtype != torch.uint8 or tuple(mk.shape) != tuple(im.shape[:2]) or not mk.is_cuda:
                raise ValueError(f"{who}: mask must be a CUDA uint8 [H, W] tensor of the image's size")
            if mk.stride(1) != 1:
                mk = mk.contiguous()
            keep.append(mk)
            d.mask, d.mask_row_stride = mk.data_ptr(), mk.stride(0)
        else:
            d.mask, d.mask_row_stride = None, 0
    return descs, keep, images[0].device


def _int_array(a, shape, who: str, what: str) -> np.ndarray:
    """An integer array or tensor of exactly `shape` (None = any length) whose values fit int32 -> contiguous int32 numpy."""
    a = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    if a.dtype.kind not in "iu" or a.ndim != len(shape) or any(n is not None and n != m for n, m in zip(shape, a.shape)):
        raise ValueError(f"{who}: {what} must be an integer array of shape [{', '.join('B' if n is None else str(n) for n in shape)}]")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"{who}: {what} values must fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def _table(lut, B: int, dev, keep, who: str):
    """The optional CUDA uint8 [B, 3, 256] table -> its device address or None; the tensor joins `keep`."""
    if lut is None:
        return None
    if not isinstance(lut, torch.Tensor) or not lut.is_cuda or lut.dtype != torch.uint8 or tuple(lut.shape) != (B, 3, 256) or lut.device != dev:
        raise ValueError(f"{who}: lut must be a CUDA uint8 [{B}, 3, 256] tensor on the images' device")
    keep.append(lut.contiguous())
    return keep[-1].data_ptr()


def _run(B: int, img_size: int, dev, keep, launch, name: str):
    """Allocate (imgs [B,3,S,S], masks [B,1,S,S]), call launch(image address, mask address, stream) -> status of entry point `name`."""
    out = torch.empty(B, 3, img_size, img_size, device=dev, dtype=torch.float32)
    out_m = torch.empty(B, 1, img_size, img_size, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev)
    L.check(launch(out.data_ptr(), out_m.data_ptr(), C.c_void_p(stream.cuda_stream)), name)
    for t in keep:   # the launch is asynchronous: keep the sources alive until the stream has consumed them
        t.record_stream(stream)
    return out, out_m


def _split(ranges: dict, who: str, geo_keys):
    """The keyword arguments of `*_samples` -> those of the geometry draw, `sample_photometric` and the label move; others are an error."""
    parts = [{k: ranges.pop(k) for k in keys if k in ranges}
             for keys in (geo_keys, ("brightness", "contrast", "gamma"), ("min_px", "min_area_ratio", "max_aspect"))]
    if ranges:
        raise TypeError(f"{who}: unknown arguments {sorted(ranges)}")
    return parts


_INT32_P = C.POINTER(C.c_int32)


def letterbox_batch(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]] = None, img_size: int = 640):
    """images: decoded BGR uint8 [H0, W0, 3] CUDA tensors (any sizes); masks: uint8 [H0, W0] CUDA tensors or None.
    Returns (imgs [B,3,S,S] f32 RGB in [0,1], masks [B,1,S,S] f32 {0,1}, scales list[float]) -- `img_t`, `mask_t` and
    `scale` of dataset_btxrdv2.py:153-166 for every sample, stacked like `collate_fn` (:264-265)."""
    lib = L.load()
    descs, keep, dev = _descriptors(images, masks, "letterbox_batch")
    B = len(images)
    scales = (C.c_double * B)()
    out, out_m = _run(B, img_size, dev, keep, lambda x, m, st: lib.mtbt_letterbox_batch(descs, B, img_size, x, m, scales, st), "mtbt_letterbox_batch")
    return out, out_m, [float(s) for s in scales]


def transform_yolo_labels(rows: Sequence[Sequence[float]], W0: int, H0: int, scale: float, img_size: int) -> List[List[float]]:
    """YOLO-txt rows (cls, xc, yc, w, h normalised to the ORIGINAL image) -> the reference's per-sample `det_rows`
    [0.0, cls, xc, yc, w, h] normalised to the letterboxed S x S image (dataset_btxrdv2.py:173-245): boxes with
    non-positive size, under one pixel after scaling, or under 1/S after clamping to [0, 1] are dropped."""
    out = []
    min_norm = 1.0 / img_size
    clip = lambda v: min(max(v, 0.0), 1.0)
    for r in rows:
        if len(r) < 5:
            continue
        cls, xc, yc, w, h = (float(v) for v in r[:5])
        if w <= 0 or h <= 0:
            continue
        axc, ayc, aw, ah = xc * W0, yc * H0, w * W0, h * H0
        x1, y1, x2, y2 = (axc - aw / 2) * scale, (ayc - ah / 2) * scale, (axc + aw / 2) * scale, (ayc + ah / 2) * scale
        fw, fh = x2 - x1, y2 - y1
        if fw < 1.0 or fh < 1.0:
            continue
        cxn, cyn, wn, hn = ((x1 + x2) / 2) / img_size, ((y1 + y2) / 2) / img_size, fw / img_size, fh / img_size
        nx1, ny1, nx2, ny2 = clip(cxn - wn / 2), clip(cyn - hn / 2), clip(cxn + wn / 2), clip(cyn + hn / 2)
        cw, ch = nx2 - nx1, ny2 - ny1
        if cw < min_norm or ch < min_norm:
            continue
        out.append([0.0, cls, (nx1 + nx2) / 2, (ny1 + ny2) / 2, cw, ch])
    return out


def collate_boxes(per_sample_rows: Sequence[Sequence[Sequence[float]]], device=None) -> torch.Tensor:
    """`collate_fn` (:267-281): stamp the batch index into column 0 and concatenate -> [N, 6] float32."""
    rows = []
    for i, sample in enumerate(per_sample_rows):
        for r in sample:
            rows.append([float(i)] + [float(v) for v in r[1:6]])
    t = torch.tensor(rows, dtype=torch.float32) if rows else torch.zeros((0, 6), dtype=torch.float32)
    return t.to(device) if device is not None else t


# ---- contrast-limited adaptive histogram equalisation of the raw images (the project's own definition, modelled on cv2's CLAHE) ----
def _grid(grid, who: str):
    gx, gy = (int(v) for v in grid)
    if not (1 <= gx <= 16 and 1 <= gy <= 16):
        raise ValueError(f"{who}: grid = (gx, gy) must lie in [1, 16] per axis")
    return gx, gy


def clahe_clip(clip_limit: float, H: int, W: int, grid=(8, 8)) -> int:
    """cv2's integer clip of a `clipLimit` for an H x W image on a (gx, gy) grid: 0 (no clipping) if clip_limit <= 0, else
    max(1, int(clip_limit * area / 256)) with area = ceil(W / gx) * ceil(H / gy), in Python floats.  This integer is all the library sees."""
    gx, gy = _grid(grid, "clahe_clip")
    area = -(-int(W) // gx) * -(-int(H) // gy)
    return 0 if clip_limit <= 0 else max(1, int(float(clip_limit) * area / 256))


def _row_strided(t: torch.Tensor) -> bool:
    """Pixels of a row contiguous and the rows apart by at least a row: what the library addresses without a copy."""
    ch = 1 if t.dim() == 2 else 3
    inner = t.stride(1) == 1 if t.dim() == 2 else (t.stride(2) == 1 and t.stride(1) == 3)
    return inner and (t.shape[0] == 1 or t.stride(0) >= t.shape[1] * ch)


def clahe_batch(images: Sequence[torch.Tensor], clip_limit=2.0, grid=(8, 8), out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """Contrast-limited adaptive histogram equalisation of raw images at their own resolution, on the device (include/mtbt_hip.h
    `mtbt_clahe_batch` states the rule: this project's own, modelled step for step on cv2's `createCLAHE(clipLimit, tileGridSize)`).
    images: uint8 [H, W] or [H, W, 3] CUDA tensors of any sizes, mixed freely, row-strided views included (anything else is copied);
    a three-channel image gets ONE curve per tile, built from (c0 + 2 c1 + c2 + 2) >> 2 and applied to each channel.  clip_limit: a
    scalar or one value per image (<= 0 equalises without clipping); None for an image returns that tensor itself, untouched.
    grid = (gx, gy) tiles per axis, each in [1, 16] and no more than the image has pixels on that axis.  out: None (new tensors) or one
    uint8 CUDA tensor per image of the image's shape, row-strided, written in its first W * channels bytes per row only; `out=images`
    works in place.  Returns the list of equalised tensors.  Three launches per <= 32 images, asynchronous, no CPU path."""
    lib = L.load()
    B = len(images)
    if B == 0:
        raise ValueError("clahe_batch: empty batch")
    gx, gy = _grid(grid, "clahe_batch")
    limits = list(clip_limit) if isinstance(clip_limit, (list, tuple, np.ndarray)) else [clip_limit] * B
    if len(limits) != B or (out is not None and len(out) != B):
        raise ValueError("clahe_batch: one clip limit and one output per image")
    result, keep, items = list(images), [], []
    dev = images[0].device
    for i, im in enumerate(images):
        if limits[i] is None:
            continue
        if not isinstance(im, torch.Tensor) or not im.is_cuda or im.device != dev:
            raise RuntimeError("clahe_batch: expected CUDA/HIP tensors on one MI355X (no CPU path)")
        if im.dtype != torch.uint8 or not (im.dim() == 2 or (im.dim() == 3 and im.shape[2] == 3)):
            raise ValueError("clahe_batch: images must be uint8 [H, W] or [H, W, 3]")
        H, W = int(im.shape[0]), int(im.shape[1])
        if H < gy or W < gx:
            raise ValueError(f"clahe_batch: image {i} ({H} x {W}) has fewer pixels than the grid {gx} x {gy} has tiles")
        dst = torch.empty(tuple(im.shape), device=dev, dtype=torch.uint8) if out is None else out[i]
        if out is not None and (not isinstance(dst, torch.Tensor) or not dst.is_cuda or dst.device != dev or dst.dtype != torch.uint8
                                or tuple(dst.shape) != tuple(im.shape) or not _row_strided(dst)):
            raise ValueError(f"clahe_batch: out[{i}] must be a row-strided CUDA uint8 tensor of the image's shape")
        src = im if _row_strided(im) else im.contiguous()
        keep += [src, dst]
        items.append((src, dst, clahe_clip(float(limits[i]), H, W, (gx, gy))))
        result[i] = dst
    if not items:
        return result
    n = len(items)
    descs = (L.ClaheImage * n)()
    for d, (src, dst, clip) in zip(descs, items):
        d.src, d.dst, d.height, d.width, d.channels, d.clip = src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1], 1 if src.dim() == 2 else 3, clip
        d.src_row_stride = src.stride(0) if src.shape[0] > 1 else src.shape[1] * d.channels
        d.dst_row_stride = dst.stride(0) if dst.shape[0] > 1 else dst.shape[1] * d.channels
    workspace, nbytes = L.workspace(lib.mtbt_clahe_workspace_bytes, descs, n, gx, gy, device=dev, what="mtbt_clahe_workspace_bytes")
    stream = torch.cuda.current_stream(dev)
    L.check(lib.mtbt_clahe_batch(descs, n, gx, gy, workspace.data_ptr(), nbytes, C.c_void_p(stream.cuda_stream)), "mtbt_clahe_batch")
    for t in keep:   # the launches are asynchronous: keep the buffers alive until the stream has consumed them
        t.record_stream(stream)
    return result


def sample_clahe(B: int, rng: np.random.Generator, *, prob: float = 0.5, clip=(1.0, 4.0)) -> list:
    """Draw, per image, whether it is equalised (probability prob) and its clip limit ~ U(clip): a list of B floats or None, the
    `clip_limit` of `clahe_batch`.  Two vectors of B draws in that order whatever prob is, so a seeded generator gives the same list again."""
    on = rng.random(B) < prob
    c = rng.uniform(clip[0], clip[1], B)
    return [float(c[i]) if on[i] else None for i in range(B)]


def _equalised(images, rng: np.random.Generator, clahe: Optional[dict]):
    """The `clahe=dict(prob=, clip=, grid=)` option of the `*_samples` functions: every source image is equalised at most once, at its own
    resolution, before any resampling; the draws (`sample_clahe`) are the last ones.  None draws nothing and returns the images."""
    if clahe is None:
        return images
    opts = dict(clahe)
    grid = opts.pop("grid", (8, 8))
    return clahe_batch(images, sample_clahe(len(images), rng, **opts), grid)


# ---- training augmentation (the project's own definition: the reference has none) ------------------------------------------
GEOM_FIELDS = 8  # new_w, new_h, off_x, off_y, orient (bit 0 flip x, bit 1 flip y, bit 2 transpose), 3 reserved zeros


def augment_batch(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]], geom, lut: Optional[torch.Tensor] = None,
                  img_size: int = 640):
    """`letterbox_batch` with the geometry given per image: geom int [B, 8] rows (new_w, new_h, off_x, off_y, orient, 0, 0, 0) as
    `letterbox_geometry` / `sample_geometry` return them, lut an optional CUDA uint8 [B, 3, 256] table (BGR order, `photometric_lut`).
    Returns (imgs [B,3,S,S] f32 RGB in [0,1], masks [B,1,S,S] f32 {0,1}); one launch per <= 32 images, no CPU path."""
    lib = L.load()
    descs, keep, dev = _descriptors(images, masks, "augment_batch")
    B = len(images)
    g = _int_array(geom, (B, GEOM_FIELDS), "augment_batch", "geom")
    table = _table(lut, B, dev, keep, "augment_batch")
    return _run(B, img_size, dev, keep, lambda x, m, st: lib.mtbt_augment_batch(descs, B, img_size, g.ctypes.data_as(_INT32_P), GEOM_FIELDS, table, x, m, st),
                "mtbt_augment_batch")


def letterbox_geometry(sizes: Sequence[Sequence[int]], img_size: int) -> np.ndarray:
    """sizes: (H0, W0) per image.  The identity parameters: the reference's new_w / new_h (dataset_btxrdv2.py:114-117), zero
    offsets, orient 0 -- `augment_batch` with them and no table is `letterbox_batch`."""
    geom = np.zeros((len(sizes), GEOM_FIELDS), dtype=np.int32)
    for i, (H0, W0) in enumerate(sizes):
        s = img_size / max(H0, W0)
        geom[i, 0], geom[i, 1] = max(1, int(W0 * s)), max(1, int(H0 * s))
    return geom


def sample_geometry(sizes: Sequence[Sequence[int]], img_size: int, rng: np.random.Generator, *, scale=(0.5, 1.5), aspect: float = 0.0,
                    fliplr: float = 0.5, flipud: float = 0.0, transpose: float = 0.0, place: str = "random") -> np.ndarray:
    """Draw one geometry row per image.  new_w = max(1, int(W0 * s * g * a)), new_h = max(1, int(H0 * s * g / a)) with
    s = S / max(H0, W0), g ~ U(scale), a = exp(U(-aspect, aspect)); each orientation bit is set with its probability;
    place "topleft" puts the oriented image at (0, 0), "random" at floor(u * (S - q)) per axis, u ~ U[0, 1): a random position while
    the canvas has padding on that axis, a random crop window once the image is larger than the canvas.  The draws come in a fixed
    order (g, a, the three bits, the two offsets; one vector of B each), so a seeded generator gives the same array again."""
    if place not in ("random", "topleft"):
        raise ValueError("sample_geometry: place must be 'random' or 'topleft'")
    B = len(sizes)
    g = rng.uniform(scale[0], scale[1], B)
    a = np.exp(rng.uniform(-aspect, aspect, B))
    bits = [rng.random(B) < p for p in (fliplr, flipud, transpose)]
    u = rng.random((B, 2))
    geom = np.zeros((B, GEOM_FIELDS), dtype=np.int32)
    for i, (H0, W0) in enumerate(sizes):
        s = img_size / max(H0, W0)
        new_w = min(max(1, int(W0 * s * float(g[i]) * float(a[i]))), 32768)
        new_h = min(max(1, int(H0 * s * float(g[i]) / float(a[i]))), 32768)
        orient = int(bits[0][i]) | int(bits[1][i]) << 1 | int(bits[2][i]) << 2
        qw, qh = (new_h, new_w) if orient & 4 else (new_w, new_h)
        off_x = off_y = 0
        if place == "random":
            off_x, off_y = math.floor(float(u[i, 0]) * (img_size - qw)), math.floor(float(u[i, 1]) * (img_size - qh))
        geom[i, :5] = new_w, new_h, off_x, off_y, orient
    return geom


def photometric_lut(brightness, contrast, gamma) -> np.ndarray:
    """Per-image scalars [B] -> uint8 [B, 3, 256]: row v -> rint(255 * (contrast * ((v / 255) ** gamma - 0.5) + 0.5 + brightness))
    clipped to 0..255, in float64, the same row for the three channels.  (0, 1, 1) is the identity table."""
    b, c, g = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (brightness, contrast, gamma))
    v = np.arange(256, dtype=np.float64) / 255.0
    row = np.rint(255.0 * (c[:, None] * (v[None, :] ** g[:, None] - 0.5) + 0.5 + b[:, None]))
    row = np.clip(row, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(row[:, None, :], 3, axis=1))


def sample_photometric(B: int, rng: np.random.Generator, *, brightness: float = 0.2, contrast: float = 0.2, gamma: float = 0.2) -> np.ndarray:
    """Draw brightness ~ U(+-brightness), contrast ~ U(1 +- contrast), gamma = exp(U(+-gamma)) per image -> `photometric_lut`."""
    b = rng.uniform(-brightness, brightness, B)
    c = rng.uniform(1.0 - contrast, 1.0 + contrast, B)
    g = np.exp(rng.uniform(-gamma, gamma, B))
    return photometric_lut(b, c, g)


def augment_yolo_labels(rows: Sequence[Sequence[float]], W0: int, H0: int, geom_row, img_size: int, *, min_px: float = 2.0,
                        min_area_ratio: float = 0.1, max_aspect: float = 100.0, clip_rect=None) -> List[List[float]]:
    """YOLO-txt rows (cls, xc, yc, w, h normalised to the ORIGINAL image) -> [0.0, cls, cx, cy, w, h] normalised to the augmented
    S x S canvas of `augment_batch` under geom_row.  Corners in source pixels, times new / old per axis, through the orientation (the
    pixel map Q -> R of the kernel, inverted: transpose swap, then x -> qw - x, y -> qh - y), plus the offsets, clipped to [0, S].
    A box is dropped when a clipped side is < min_px, when clipped area / unclipped area <= min_area_ratio (mostly cropped away), or
    when its side ratio is >= max_aspect.  Python floats, like `transform_yolo_labels`.  clip_rect = (x0, y0, x1, y1) in canvas pixels
    replaces the clip to [0, S] by the clip to that rectangle (a mosaic tile, `mosaic_yolo_labels`); None is the whole canvas."""
    new_w, new_h, off_x, off_y, orient = (int(v) for v in geom_row[:5])
    qw, qh = (new_h, new_w) if orient & 4 else (new_w, new_h)
    kx, ky, S = new_w / W0, new_h / H0, float(img_size)
    rx0, ry0, rx1, ry1 = (0.0, 0.0, S, S) if clip_rect is None else (float(v) for v in clip_rect)
    clip_x = lambda v: min(max(v, rx0), rx1)
    clip_y = lambda v: min(max(v, ry0), ry1)
    out = []
    for r in rows:
        if len(r) < 5:
            continue
        cls, xc, yc, w, h = (float(v) for v in r[:5])
        if w <= 0 or h <= 0:
            continue
        x1, y1, x2, y2 = (xc - w / 2) * W0 * kx, (yc - h / 2) * H0 * ky, (xc + w / 2) * W0 * kx, (yc + h / 2) * H0 * ky
        if orient & 4:
            x1, y1, x2, y2 = y1, x1, y2, x2
        if orient & 1:
            x1, x2 = qw - x2, qw - x1
        if orient & 2:
            y1, y2 = qh - y2, qh - y1
        x1, y1, x2, y2 = x1 + off_x, y1 + off_y, x2 + off_x, y2 + off_y
        area = (x2 - x1) * (y2 - y1)
        cx1, cy1, cx2, cy2 = clip_x(x1), clip_y(y1), clip_x(x2), clip_y(y2)
        cw, ch = cx2 - cx1, cy2 - cy1
        if cw < min_px or ch < min_px or cw <= 0.0 or ch <= 0.0:
            continue
        if cw * ch / area <= min_area_ratio:
            continue
        if max(cw / ch, ch / cw) >= max_aspect:
            continue
        out.append([0.0, cls, (cx1 + cx2) / 2 / S, (cy1 + cy2) / 2 / S, cw / S, ch / S])
    return out


def augment_samples(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]],
                    rows_per_image: Sequence[Sequence[Sequence[float]]], img_size: int, rng: np.random.Generator, **ranges):
    """Draw geometry and intensity, run `augment_batch`, move the labels: (imgs [B,3,S,S], masks [B,1,S,S], gt_rows [M,6] on the
    device, batch index in column 0) -- what `TrainStep.step` takes.  `ranges` are the keyword arguments of `sample_geometry`,
    `sample_photometric` and `augment_yolo_labels`, plus clahe=dict(prob=, clip=, grid=) (`sample_clahe`, `clahe_batch`: the sources are
    equalised at their own resolution before the resample; its draws come last, so geometry, tables and labels are the same with and
    without it, and None -- the default -- draws nothing); anything else is an error."""
    clahe = ranges.pop("clahe", None)
    geo, pho, lab = _split(ranges, "augment_samples", ("scale", "aspect", "fliplr", "flipud", "transpose", "place"))
    if len(rows_per_image) != len(images):
        raise ValueError("augment_samples: one list of label rows per image")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    geom = sample_geometry(sizes, img_size, rng, **geo)
    lut = torch.from_numpy(sample_photometric(len(images), rng, **pho)).to(images[0].device)
    imgs, out_masks = augment_batch(_equalised(images, rng, clahe), masks, geom, lut, img_size)
    rows = [augment_yolo_labels(r, W0, H0, geom[i], img_size, **lab) for i, (r, (H0, W0)) in enumerate(zip(rows_per_image, sizes))]
    return imgs, out_masks, collate_boxes(rows, device=imgs.device)


# ---- four-image mosaic (the project's own definition as well) ------------------------------------------------------------------
def tile_rects(centre, img_size: int):
    """The four half-open rectangles (x0, y0, x1, y1) a centre (cx, cy) cuts an S x S canvas into, tile 0..3 (x then y)."""
    cx, cy, S = int(centre[0]), int(centre[1]), int(img_size)
    return [(0, 0, cx, cy), (cx, 0, S, cy), (0, cy, cx, S), (cx, cy, S, S)]


def mosaic_batch(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]], index, geom, centres,
                 lut: Optional[torch.Tensor] = None, img_size: int = 640):
    """B canvases of four tiles each: index int [B, 4] into `images` (repeats allowed), geom int [B, 4, 8] rows as for `augment_batch`
    with the offsets in canvas coordinates, centres int [B, 2] = (cx, cy) with 0 <= cx <= S, cx % 4 == 0, 0 <= cy <= S, lut an optional
    CUDA uint8 [B, 3, 256] table per CANVAS.  Tile t of a canvas shows, inside its rectangle (`tile_rects`), what `augment_batch` would
    draw for images[index[b, t]] under geom[b, t]; a centre of (S, S) makes the canvas `augment_batch` of tile 0.
    Returns (imgs [B,3,S,S] f32 RGB in [0,1], masks [B,1,S,S] f32 {0,1}); one launch per <= 8 canvases, no CPU path."""
    lib = L.load()
    descs, keep, dev = _descriptors(images, masks, "mosaic_batch")
    idx = _int_array(index, (None, 4), "mosaic_batch", "index")
    B = idx.shape[0]
    if B == 0:
        raise ValueError("mosaic_batch: empty batch")
    if idx.min() < 0 or idx.max() >= len(images):
        raise ValueError(f"mosaic_batch: index values must lie in [0, {len(images)})")
    g = _int_array(geom, (B, 4, GEOM_FIELDS), "mosaic_batch", "geom")
    c = _int_array(centres, (B, 2), "mosaic_batch", "centres")
    table = _table(lut, B, dev, keep, "mosaic_batch")
    # the four descriptors of every canvas, gathered in one step (the library reads them before it returns)
    tiles = np.ascontiguousarray(np.frombuffer(descs, dtype=np.uint8).reshape(len(images), C.sizeof(L.RawImage))[idx.reshape(-1)])
    return _run(B, img_size, dev, keep, lambda x, m, st: lib.mtbt_mosaic_batch(tiles.ctypes.data_as(C.POINTER(L.RawImage)), B, img_size, g.ctypes.data_as(_INT32_P),
                                                                                GEOM_FIELDS, c.ctypes.data_as(_INT32_P), table, x, m, st), "mtbt_mosaic_batch")


def sample_mosaic(sizes: Sequence[Sequence[int]], img_size: int, rng: np.random.Generator, *, prob: float = 1.0, centre=(0.25, 0.75),
                  scale=(0.5, 1.0), aspect: float = 0.0, fliplr: float = 0.5, flipud: float = 0.0, transpose: float = 0.0):
    """Draw one canvas per entry of sizes ((H0, W0) per image): (index int64 [B, 4], geom int32 [B, 4, 8], centres int32 [B, 2]) for
    `mosaic_batch`.  Canvas i is a mosaic with probability prob: image i sits in a tile drawn from 0..3, the three other tiles show images
    drawn uniformly from all B with replacement, cx = 4 * floor(u * S / 4) and cy = floor(u * S) with u ~ U(centre) each, every tile's
    new_w / new_h / orientation follow `sample_geometry`'s formula for its own image, and the oriented image (qw x qh) is placed so that
    the corner facing the centre touches it: offsets (cx - qw, cy - qh), (cx, cy - qh), (cx - qw, cy), (cx, cy) for tiles 0..3.
    Otherwise the centre is (S, S), tile 0 is image i under a `sample_geometry(place="random")` row and tiles 1..3 are image i under the
    letterbox row (drawn nowhere): `mosaic_batch` then gives `augment_batch` of tile 0.
    The draws come in a fixed order whatever prob is -- the mosaic decision (B), the own tile position (B), the other sources (B x 3),
    the centres (B x 2: x, y), then ONE `sample_geometry(place="random")` call over the 4 B tiles in canvas-major order -- so a seeded
    generator gives the same arrays again."""
    B, S = len(sizes), int(img_size)
    is_mosaic = rng.random(B) < prob
    own = rng.integers(0, 4, B)
    others = rng.integers(0, max(B, 1), (B, 3))
    u = rng.uniform(centre[0], centre[1], (B, 2))
    index = np.repeat(np.arange(B, dtype=np.int64)[:, None], 4, axis=1)
    for i in range(B):
        if is_mosaic[i]:
            index[i, [t for t in range(4) if t != own[i]]] = others[i]
    geom = sample_geometry([sizes[k] for k in index.reshape(-1)], S, rng, scale=scale, aspect=aspect, fliplr=fliplr, flipud=flipud,
                           transpose=transpose, place="random").reshape(B, 4, GEOM_FIELDS)
    centres = np.full((B, 2), S, dtype=np.int32)
    for i in range(B):
        if is_mosaic[i]:
            cx, cy = 4 * math.floor(float(u[i, 0]) * S / 4), math.floor(float(u[i, 1]) * S)
            centres[i] = cx, cy
            for t in range(4):
                new_w, new_h, orient = (int(v) for v in geom[i, t, [0, 1, 4]])
                qw, qh = (new_h, new_w) if orient & 4 else (new_w, new_h)
                geom[i, t, 2], geom[i, t, 3] = (cx if t & 1 else cx - qw), (cy if t & 2 else cy - qh)
        else:
            geom[i, 1:] = letterbox_geometry([sizes[i]], S)[0]
    return index, geom, centres


def mosaic_yolo_labels(rows_per_tile: Sequence[Sequence[Sequence[float]]], sizes_per_tile: Sequence[Sequence[int]], geom4, centre, img_size: int, *,
                       min_px: float = 2.0, min_area_ratio: float = 0.1, max_aspect: float = 100.0) -> List[List[float]]:
    """The label rows of one mosaic canvas: `augment_yolo_labels` per tile (rows and (H0, W0) of the tile's image, geom4[t]) with the clip
    to [0, S] replaced by the clip to the tile's rectangle, the same drop rules, the four tiles' rows concatenated in tile order."""
    if not (len(rows_per_tile) == len(sizes_per_tile) == len(geom4) == 4):
        raise ValueError("mosaic_yolo_labels: four tiles per canvas")
    out = []
    for rows, (H0, W0), g, rect in zip(rows_per_tile, sizes_per_tile, geom4, tile_rects(centre, img_size)):
        out += augment_yolo_labels(rows, W0, H0, g, img_size, min_px=min_px, min_area_ratio=min_area_ratio, max_aspect=max_aspect, clip_rect=rect)
    return out


def mosaic_samples(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]],
                   rows_per_image: Sequence[Sequence[Sequence[float]]], img_size: int, rng: np.random.Generator, **ranges):
    """`augment_samples` with four images per canvas: draw `sample_mosaic`, then `sample_photometric` (one table per canvas) from the one
    generator, run `mosaic_batch`, move the labels with `mosaic_yolo_labels`: (imgs [B,3,S,S], masks [B,1,S,S], gt_rows [M,6] on the
    device, batch index = canvas in column 0) -- what `TrainStep.step` takes.  `ranges` are the keyword arguments of those three functions,
    plus clahe=dict(prob=, clip=, grid=) as in `augment_samples` (one draw per IMAGE, each equalised at most once however many tiles show
    it); anything else is an error."""
    clahe = ranges.pop("clahe", None)
    geo, pho, lab = _split(ranges, "mosaic_samples", ("prob", "centre", "scale", "aspect", "fliplr", "flipud", "transpose"))
    if len(rows_per_image) != len(images):
        raise ValueError("mosaic_samples: one list of label rows per image")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    index, geom, centres = sample_mosaic(sizes, img_size, rng, **geo)
    lut = torch.from_numpy(sample_photometric(len(images), rng, **pho)).to(images[0].device)
    imgs, out_masks = mosaic_batch(_equalised(images, rng, clahe), masks, index, geom, centres, lut, img_size)
    rows = [mosaic_yolo_labels([rows_per_image[k] for k in index[i]], [sizes[k] for k in index[i]], geom[i], centres[i], img_size, **lab)
            for i in range(len(images))]
    return imgs, out_masks, collate_boxes(rows, device=imgs.device)


# ---- polygon labels (YOLO-seg rows) under the same augmentation: vertices moved on the host, rasterised at the canvas resolution ----
def _shoelace(pts) -> float:
    """Signed area of a closed polygon given as a list of (x, y)."""
    a = 0.0
    for i in range(len(pts)):
        (x1, y1), (x2, y2) = pts[i], pts[(i + 1) % len(pts)]
        a += x1 * y2 - x2 * y1
    return a / 2


def _clip_polygon(pts, rect):
    """Sutherland-Hodgman: the polygon (list of (x, y)) clipped to the rectangle (x0, y0, x1, y1); a point put on a clip line carries
    that line's coordinate exactly."""
    rx0, ry0, rx1, ry1 = rect
    for axis, bound, keep_ge in ((0, rx0, True), (0, rx1, False), (1, ry0, True), (1, ry1, False)):
        if not pts:
            break
        inside = (lambda q: q[axis] >= bound) if keep_ge else (lambda q: q[axis] <= bound)
        out = []
        for i in range(len(pts)):
            a, b = pts[i - 1], pts[i]
            if inside(a) != inside(b):
                t = (bound - a[axis]) / (b[axis] - a[axis])
                other = a[1 - axis] + (b[1 - axis] - a[1 - axis]) * t
                out.append((bound, other) if axis == 0 else (other, bound))
            if inside(b):
                out.append(b)
        pts = out
    return pts


def _polygon_row(cls: float, pts, rect, S: float, min_px: float, min_area_ratio: float, max_aspect: float):
    """The label row of a moved polygon (list of (x, y) in canvas pixels), or None when it is dropped: clip to `rect` (Sutherland-Hodgman),
    take the clipped polygon's box, apply the three drop rules.  The one tail of `augment_polygons`, `affine_polygons` and
    `affine_yolo_labels`."""
    area = abs(_shoelace(pts))
    if not area > 0.0:
        return None
    cl = _clip_polygon(pts, rect)
    if len(cl) < 3:
        return None
    cx1, cx2 = min(q[0] for q in cl), max(q[0] for q in cl)
    cy1, cy2 = min(q[1] for q in cl), max(q[1] for q in cl)
    cw, ch = cx2 - cx1, cy2 - cy1
    if cw < min_px or ch < min_px or cw <= 0.0 or ch <= 0.0:
        return None
    if abs(_shoelace(cl)) / area <= min_area_ratio:
        return None
    if max(cw / ch, ch / cw) >= max_aspect:
        return None
    return [0.0, cls, (cx1 + cx2) / 2 / S, (cy1 + cy2) / 2 / S, cw / S, ch / S]


def augment_polygons(rows: Sequence[Sequence[float]], W0: int, H0: int, geom_row, img_size: int, *, min_px: float = 2.0,
                     min_area_ratio: float = 0.1, max_aspect: float = 100.0, clip_rect=None):
    """YOLO-seg rows (cls, x1, y1, x2, y2, ... normalised to the ORIGINAL image) -> a list of (row6, vertices) on the augmented S x S
    canvas of `augment_batch` under geom_row.  Every vertex goes through exactly the map `augment_yolo_labels` applies to box corners
    (times new / old per axis, transpose swap, x -> qw - x, y -> qh - y, plus the offsets; Python floats).  `vertices` is float64
    [n, 2] in canvas pixels, NOT clipped: the rasteriser clips (`postprocess.fill_polygons`).  row6 = [0.0, cls, cx, cy, w, h],
    normalised by S, is the bounding box of the polygon clipped (Sutherland-Hodgman) to clip_rect, or to [0, S]^2 when that is None.
    A polygon is dropped when it has fewer than 3 vertices or zero area, when a clipped box side is < min_px, when
    |area of the clipped polygon| / |area of the polygon| <= min_area_ratio (shoelace), or when the box side ratio is >= max_aspect:
    the rules of `augment_yolo_labels`, which a rectangle given as four vertices reproduces."""
    new_w, new_h, off_x, off_y, orient = (int(v) for v in geom_row[:5])
    qw, qh = (new_h, new_w) if orient & 4 else (new_w, new_h)
    kx, ky, S = new_w / W0, new_h / H0, float(img_size)
    rect = (0.0, 0.0, S, S) if clip_rect is None else tuple(float(v) for v in clip_rect)
    out = []
    for r in rows:
        n = (len(r) - 1) // 2
        if n < 3:
            continue
        cls = float(r[0])
        pts = []
        for i in range(n):
            x, y = float(r[1 + 2 * i]) * W0 * kx, float(r[2 + 2 * i]) * H0 * ky
            if orient & 4:
                x, y = y, x
            if orient & 1:
                x = qw - x
            if orient & 2:
                y = qh - y
            pts.append((x + off_x, y + off_y))
        row6 = _polygon_row(cls, pts, rect, S, min_px, min_area_ratio, max_aspect)
        if row6 is not None:
            out.append((row6, np.asarray(pts, dtype=np.float64).reshape(n, 2)))
    return out


def mosaic_polygons(rows_per_tile: Sequence[Sequence[Sequence[float]]], sizes_per_tile: Sequence[Sequence[int]], geom4, centre, img_size: int, *,
                    min_px: float = 2.0, min_area_ratio: float = 0.1, max_aspect: float = 100.0):
    """The polygons of one mosaic canvas: `augment_polygons` per tile, clipped to the tile's rectangle (`tile_rects`), the four tiles
    concatenated in tile order -> a list of (row6, vertices, rect); `rect` is what the rasteriser clips that polygon's plane to."""
    if not (len(rows_per_tile) == len(sizes_per_tile) == len(geom4) == 4):
        raise ValueError("mosaic_polygons: four tiles per canvas")
    out = []
    for rows, (H0, W0), g, rect in zip(rows_per_tile, sizes_per_tile, geom4, tile_rects(centre, img_size)):
        out += [(row6, v, rect) for row6, v in augment_polygons(rows, W0, H0, g, img_size, min_px=min_px, min_area_ratio=min_area_ratio,
                                                                max_aspect=max_aspect, clip_rect=rect)]
    return out


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    """A host tensor -> the device through pinned memory, asynchronously: the host does not wait for the stream."""
    return t.pin_memory().to(dev, non_blocking=True) if t.numel() else t.to(dev)


def _seg_outputs(per_canvas, canvas_rects, img_size: int, dev):
    """per_canvas: for every canvas its list of (row6, vertices, rect); canvas_rects: for every canvas the G rectangles its polygons are
    clipped to (one for a plain canvas, the four tiles of a mosaic) -> (masks [B,1,S,S], gt_rows [M,6], inst) of the `*_samples_seg`
    functions: one fill for the M instance planes, one for the B x G unions of the polygons that share a rectangle."""
    S, B, G = int(img_size), len(per_canvas), len(canvas_rects[0])
    items = [(i, it) for i, canvas in enumerate(per_canvas) for it in canvas]
    gt_rows = _upload(collate_boxes([[it[0] for it in canvas] for canvas in per_canvas]), dev)
    planes = fill_polygons([it[1] for _, it in items], S, S, clip=np.asarray([it[2] for _, it in items], dtype=np.int32).reshape(-1, 4), device=dev)
    inst = {"planes": planes, "image": _upload(torch.tensor([i for i, _ in items], dtype=torch.int64), dev),
            "labels": _upload(torch.tensor([int(it[0][1]) for _, it in items], dtype=torch.int64), dev)}
    groups = [[it[1] for it in canvas if tuple(it[2]) == tuple(rect)] for canvas, rects in zip(per_canvas, canvas_rects) for rect in rects]
    union = fill_polygons(groups, S, S, clip=np.asarray(canvas_rects, dtype=np.int32).reshape(-1, 4), device=dev).view(B, G, S, -1)
    merged = union[:, 0]
    for g in range(1, G):
        merged = merged | union[:, g]
    return unpack_masks(merged, S).to(torch.float32).unsqueeze(1), gt_rows, inst


def augment_samples_seg(images: Sequence[torch.Tensor], seg_rows_per_image: Sequence[Sequence[Sequence[float]]], img_size: int,
                        rng: np.random.Generator, **ranges):
    """`augment_samples` for polygon labels: seg_rows_per_image holds YOLO-seg rows (cls, x1, y1, x2, y2, ...) per image.  The generator
    is consumed exactly as `augment_samples` consumes it (the same seed gives the same `imgs`, bit for bit); the image work is
    `augment_batch` without masks; the vertices are moved on the host (`augment_polygons`) and rasterised at the canvas resolution
    (`postprocess.fill_polygons`).  Returns (imgs [B,3,S,S], masks [B,1,S,S] float32 {0,1}: the union of each canvas's surviving
    polygons, gt_rows [M,6] on the device, inst = dict(planes uint8 [M,S,pitch], image int64 [M], labels int64 [M]), row for row with
    gt_rows).  clahe=dict(prob=, clip=, grid=) as in `augment_samples`.  copy_paste=dict(...) holds the keyword arguments of
    `sample_copy_paste`: its draws come after every other draw, CLAHE's included, and `copy_paste_batch` then lays the drawn instances of
    other canvases on each canvas -- the four outputs are then `copy_paste_batch`'s (M + P rows; inst gains area, area_before, boxes).
    None -- the default -- draws nothing and changes nothing.  Nothing synchronises with the host."""
    clahe, copy_paste = ranges.pop("clahe", None), ranges.pop("copy_paste", None)
    geo, pho, lab = _split(ranges, "augment_samples_seg", ("scale", "aspect", "fliplr", "flipud", "transpose", "place"))
    if len(seg_rows_per_image) != len(images):
        raise ValueError("augment_samples_seg: one list of label rows per image")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    geom = sample_geometry(sizes, img_size, rng, **geo)
    lut = _upload(torch.from_numpy(sample_photometric(len(images), rng, **pho)), images[0].device)
    imgs, _ = augment_batch(_equalised(images, rng, clahe), None, geom, lut, img_size)
    whole = (0, 0, int(img_size), int(img_size))
    per_canvas = [[(row6, v, whole) for row6, v in augment_polygons(r, W0, H0, geom[i], img_size, **lab)]
                  for i, (r, (H0, W0)) in enumerate(zip(seg_rows_per_image, sizes))]
    return _pasted((imgs,) + _seg_outputs(per_canvas, [[whole]] * len(images), img_size, imgs.device), per_canvas, img_size, rng, copy_paste)


def mosaic_samples_seg(images: Sequence[torch.Tensor], seg_rows_per_image: Sequence[Sequence[Sequence[float]]], img_size: int,
                       rng: np.random.Generator, **ranges):
    """`mosaic_samples` for polygon labels, as `augment_samples_seg` is to `augment_samples`: the same draws, `mosaic_batch` without
    masks, `mosaic_polygons` per canvas.  Every instance plane is clipped to its tile, and so is its share of the canvas mask.
    clahe=dict(prob=, clip=, grid=) as in `mosaic_samples`; copy_paste=dict(...) as in `augment_samples_seg` (pastes are NOT clipped to a tile)."""
    clahe, copy_paste = ranges.pop("clahe", None), ranges.pop("copy_paste", None)
    geo, pho, lab = _split(ranges, "mosaic_samples_seg", ("prob", "centre", "scale", "aspect", "fliplr", "flipud", "transpose"))
    if len(seg_rows_per_image) != len(images):
        raise ValueError("mosaic_samples_seg: one list of label rows per image")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    index, geom, centres = sample_mosaic(sizes, img_size, rng, **geo)
    lut = _upload(torch.from_numpy(sample_photometric(len(images), rng, **pho)), images[0].device)
    imgs, _ = mosaic_batch(_equalised(images, rng, clahe), None, index, geom, centres, lut, img_size)
    per_canvas = [mosaic_polygons([seg_rows_per_image[k] for k in index[i]], [sizes[k] for k in index[i]], geom[i], centres[i], img_size, **lab)
                  for i in range(len(images))]
    return _pasted((imgs,) + _seg_outputs(per_canvas, [tile_rects(c, img_size) for c in centres], img_size, imgs.device), per_canvas, img_size, rng, copy_paste)


# ---- affine augmentation: rotation and shear (the project's own definition: include/mtbt_hip.h `mtbt_warp_batch`) ----------------
COEF_FIELDS = 8  # a, b, c, d, e, f (the inverse map in 1/65536 source px: X = a dx + b dy + c, Y = d dx + e dy + f), 2 reserved zeros
_INT64_P = C.POINTER(C.c_int64)


def _coef_array(coef, B: Optional[int], who: str) -> np.ndarray:
    """An integer array or tensor of shape [B, 8] (None = any B) -> contiguous int64 numpy."""
    a = np.asarray(coef.cpu() if isinstance(coef, torch.Tensor) else coef)
    if a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != COEF_FIELDS or (B is not None and a.shape[0] != B):
        raise ValueError(f"{who}: coef must be an integer array of shape [B, {COEF_FIELDS}]")
    return np.ascontiguousarray(a, dtype=np.int64)


def warp_batch(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]], coef, lut: Optional[torch.Tensor] = None,
               img_size: int = 640):
    """One canvas per image under an affine map: coef int64 [B, 8] rows (a, b, c, d, e, f, 0, 0) as `affine_coefficients` returns them --
    the INVERSE map, canvas pixel -> source position in 1/65536 px -- lut an optional CUDA uint8 [B, 3, 256] table (BGR order,
    `photometric_lut`).  The rule (fixed-point position reduced to 1/32 px, 2 x 2 taps, nearest mask, 114/255 and 0 outside the source)
    is stated in include/mtbt_hip.h `mtbt_warp_batch`; it does not average areas, so a map that shrinks by more than 2 aliases.
    Returns (imgs [B,3,S,S] f32 RGB in [0,1], masks [B,1,S,S] f32 {0,1}); one launch per <= 32 canvases, no CPU path."""
    lib = L.load()
    descs, keep, dev = _descriptors(images, masks, "warp_batch")
    B = len(images)
    k = _coef_array(coef, B, "warp_batch")
    table = _table(lut, B, dev, keep, "warp_batch")
    return _run(B, img_size, dev, keep, lambda x, m, st: lib.mtbt_warp_batch(descs, B, img_size, k.ctypes.data_as(_INT64_P), COEF_FIELDS, table, x, m, st),
                "mtbt_warp_batch")


def affine_coefficients(forward) -> np.ndarray:
    """forward: float64 [B, 2, 3] (or one [2, 3]) matrices that take source EDGE coordinates (pixel x covers [x, x + 1): the coordinates of
    the label rows times W0, H0) to canvas edge coordinates -> the int64 [B, 8] rows of `warp_batch`.  Each matrix is inverted in float64,
    the pixel-centre convention is folded into the offsets (source_index = inv . (dx + 0.5, dy + 0.5) - 0.5), and the six numbers are
    multiplied by 65536 and rounded (`np.rint`).  ValueError on a singular (or non-finite) matrix and on a coefficient outside the
    library's limits (|a|, |b|, |d|, |e| <= 2^26, |c|, |f| <= 2^47)."""
    F = np.asarray(forward, dtype=np.float64)
    F = F.reshape(1, 2, 3) if F.ndim == 2 else F
    if F.ndim != 3 or F.shape[1:] != (2, 3):
        raise ValueError("affine_coefficients: forward must be float64 [B, 2, 3]")
    coef = np.zeros((F.shape[0], COEF_FIELDS), dtype=np.int64)
    for i, M in enumerate(F):
        det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        if not np.isfinite(M).all() or not np.isfinite(det) or det == 0.0:
            raise ValueError(f"affine_coefficients: matrix {i} is singular")
        ia, ib, id_, ie = M[1, 1] / det, -M[0, 1] / det, -M[1, 0] / det, M[0, 0] / det
        ic, if_ = -(ia * M[0, 2] + ib * M[1, 2]), -(id_ * M[0, 2] + ie * M[1, 2])
        row = np.array([ia, ib, ic + 0.5 * (ia + ib) - 0.5, id_, ie, if_ + 0.5 * (id_ + ie) - 0.5]) * 65536.0
        if not np.isfinite(row).all() or np.abs(row[[0, 1, 3, 4]]).max() > L.WARP_LIN_MAX or np.abs(row[[2, 5]]).max() > L.WARP_OFF_MAX:
            raise ValueError(f"affine_coefficients: matrix {i} gives coefficients {row.tolist()} outside the library's limits "
                             f"(2^26 for a, b, d, e; 2^47 for c, f): the map shrinks the source too far or is nearly singular")
        coef[i, :6] = np.rint(row).astype(np.int64)
    return coef


def affine_forward(coef) -> np.ndarray:
    """int64 [B, 8] coefficient rows -> float64 [B, 2, 3]: the inverse of the INTEGER map the pixels use, back in edge coordinates (source
    edge -> canvas edge).  Labels are moved by `affine_forward(affine_coefficients(F))`, not by F: they follow the pixels.  The two differ
    by the 2^-17 rounding of each coefficient, a few 2^-16 S canvas pixels at most.  ValueError when the integer map is singular."""
    k = _coef_array(coef, None, "affine_forward").astype(np.float64) / 65536.0
    out = np.zeros((k.shape[0], 2, 3), dtype=np.float64)
    for i, (a, b, c, d, e, f) in enumerate(k[:, :6]):
        det = a * e - b * d
        if det == 0.0:
            raise ValueError(f"affine_forward: coefficient row {i} is a singular map")
        # source_edge = A . canvas_edge + t with t = (c, f) + 0.5 - A . (0.5, 0.5); canvas_edge = A^-1 . (source_edge - t)
        tx, ty = c + 0.5 - 0.5 * (a + b), f + 0.5 - 0.5 * (d + e)
        fa, fb, fd, fe = e / det, -b / det, -d / det, a / det
        out[i] = [[fa, fb, -(fa * tx + fb * ty)], [fd, fe, -(fd * tx + fe * ty)]]
    return out


def sample_affine(sizes: Sequence[Sequence[int]], img_size: int, rng: np.random.Generator, *, scale=(0.5, 1.5), aspect: float = 0.0,
                  degrees: float = 10.0, shear: float = 0.0, translate: float = 0.1, fliplr: float = 0.5, flipud: float = 0.0) -> np.ndarray:
    """Draw one forward matrix per image, float64 [B, 2, 3], source edge coordinates -> canvas edge coordinates:
        F = T(S/2 + tx S, S/2 + ty S) . R(theta) . Sh(tan sx, tan sy) . diag(+-kx, +-ky) . T(-W0/2, -H0/2)
    with kx = s g a, ky = s g / a, s = S / max(H0, W0), g ~ U(scale), a = exp(U(+-aspect)), theta ~ U(+-degrees), sx, sy ~ U(+-shear)
    (degrees both), tx, ty ~ U(+-translate), kx negated with probability fliplr and ky with probability flipud;
    R = [[cos, -sin], [sin, cos]], Sh = [[1, tan sx], [tan sy, 1]].  The image's centre lands on the canvas centre plus the translation.
    The draws come in a fixed order, one vector of B each -- g, a, theta, sx, sy, tx, ty, the fliplr bits, the flipud bits -- so a seeded
    generator gives the same array again."""
    B, S = len(sizes), float(img_size)
    g = rng.uniform(scale[0], scale[1], B)
    a = np.exp(rng.uniform(-aspect, aspect, B))
    theta = np.deg2rad(rng.uniform(-degrees, degrees, B))
    sx, sy = np.deg2rad(rng.uniform(-shear, shear, B)), np.deg2rad(rng.uniform(-shear, shear, B))
    tx, ty = rng.uniform(-translate, translate, B), rng.uniform(-translate, translate, B)
    lr, ud = rng.random(B) < fliplr, rng.random(B) < flipud
    out = np.zeros((B, 2, 3), dtype=np.float64)
    for i, (H0, W0) in enumerate(sizes):
        s = S / max(H0, W0)
        kx, ky = s * g[i] * a[i] * (-1.0 if lr[i] else 1.0), s * g[i] / a[i] * (-1.0 if ud[i] else 1.0)
        rot = np.array([[math.cos(theta[i]), -math.sin(theta[i])], [math.sin(theta[i]), math.cos(theta[i])]])
        lin = rot @ np.array([[1.0, math.tan(sx[i])], [math.tan(sy[i]), 1.0]]) @ np.diag([kx, ky])
        out[i, :, :2] = lin
        out[i, :, 2] = np.array([S / 2 + tx[i] * S, S / 2 + ty[i] * S]) - lin @ np.array([W0 / 2, H0 / 2])
    return out


def affine_polygons(rows: Sequence[Sequence[float]], W0: int, H0: int, forward_row, img_size: int, *, min_px: float = 2.0,
                    min_area_ratio: float = 0.1, max_aspect: float = 100.0, clip_rect=None):
    """`augment_polygons` under an affine map: YOLO-seg rows (cls, x1, y1, x2, y2, ... normalised to the ORIGINAL image) -> a list of
    (row6, vertices) on the S x S canvas of `warp_batch`.  forward_row is one float64 [2, 3] matrix of `affine_forward` (use that, not the
    matrix the coefficients were made from: labels follow the integer map).  Every vertex (x W0, y H0) goes through the matrix exactly and
    is NOT clipped -- the rasteriser clips; row6 is the box of the polygon clipped to clip_rect or [0, S]^2, under the drop rules of
    `augment_polygons`.  The box of a rotated polygon is tight: polygon rows do not grow under rotation, box rows (`affine_yolo_labels`) do."""
    M = np.asarray(forward_row, dtype=np.float64).reshape(2, 3)
    (fa, fb, fc), (fd, fe, ff) = ((float(v) for v in r) for r in M)
    S = float(img_size)
    rect = (0.0, 0.0, S, S) if clip_rect is None else tuple(float(v) for v in clip_rect)
    out = []
    for r in rows:
        n = (len(r) - 1) // 2
        if n < 3:
            continue
        pts = []
        for i in range(n):
            x, y = float(r[1 + 2 * i]) * W0, float(r[2 + 2 * i]) * H0
            pts.append((fa * x + fb * y + fc, fd * x + fe * y + ff))
        row6 = _polygon_row(float(r[0]), pts, rect, S, min_px, min_area_ratio, max_aspect)
        if row6 is not None:
            out.append((row6, np.asarray(pts, dtype=np.float64).reshape(n, 2)))
    return out


def affine_yolo_labels(rows: Sequence[Sequence[float]], W0: int, H0: int, forward_row, img_size: int, *, min_px: float = 2.0,
                       min_area_ratio: float = 0.1, max_aspect: float = 100.0, clip_rect=None) -> List[List[float]]:
    """`augment_yolo_labels` under an affine map: YOLO-txt rows (cls, xc, yc, w, h) -> [0.0, cls, cx, cy, w, h] on the canvas of
    `warp_batch`.  Each box goes through `affine_polygons` as its four corners, so its row is the axis-aligned hull of the rotated
    rectangle, clipped, under the same drop rules.  Boxes therefore GROW under rotation (a w x h box turned by 45 degrees has sides
    (w + h) / sqrt 2, and the hull of an already loose box is looser still); polygon rows do not -- prefer them when `degrees` is large."""
    out = []
    for r in rows:
        if len(r) < 5:
            continue
        cls, xc, yc, w, h = (float(v) for v in r[:5])
        if w <= 0 or h <= 0:
            continue
        x1, y1, x2, y2 = xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2
        out += [row6 for row6, _ in affine_polygons([[cls, x1, y1, x2, y1, x2, y2, x1, y2]], W0, H0, forward_row, img_size, min_px=min_px,
                                                    min_area_ratio=min_area_ratio, max_aspect=max_aspect, clip_rect=clip_rect)]
    return out


_AFFINE_KEYS = ("scale", "aspect", "degrees", "shear", "translate", "fliplr", "flipud")


def affine_samples(images: Sequence[torch.Tensor], masks: Optional[Sequence[Optional[torch.Tensor]]],
                   rows_per_image: Sequence[Sequence[Sequence[float]]], img_size: int, rng: np.random.Generator, **ranges):
    """`augment_samples` with rotation and shear: draw `sample_affine`, then `sample_photometric` from the one generator, run `warp_batch`
    on `affine_coefficients` of the draw, move the box rows with `affine_yolo_labels` under `affine_forward` of those coefficients:
    (imgs [B,3,S,S], masks [B,1,S,S], gt_rows [M,6] on the device, batch index in column 0) -- what `TrainStep.step` takes.  `ranges` are
    the keyword arguments of those three functions plus clahe=dict(prob=, clip=, grid=) as in `augment_samples` (its draws come last);
    anything else is an error.  Box rows grow under rotation (`affine_yolo_labels`); `affine_samples_seg` keeps polygon labels tight."""
    clahe = ranges.pop("clahe", None)
    geo, pho, lab = _split(ranges, "affine_samples", _AFFINE_KEYS)
    if len(rows_per_image) != len(images):
        raise ValueError("affine_samples: one list of label rows per image")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    coef = affine_coefficients(sample_affine(sizes, img_size, rng, **geo))
    forward = affine_forward(coef)
    lut = torch.from_numpy(sample_photometric(len(images), rng, **pho)).to(images[0].device)
    imgs, out_masks = warp_batch(_equalised(images, rng, clahe), masks, coef, lut, img_size)
    rows = [affine_yolo_labels(r, W0, H0, forward[i], img_size, **lab) for i, (r, (H0, W0)) in enumerate(zip(rows_per_image, sizes))]
    return imgs, out_masks, collate_boxes(rows, device=imgs.device)


def affine_samples_seg(images: Sequence[torch.Tensor], seg_rows_per_image: Sequence[Sequence[Sequence[float]]], img_size: int,
                       rng: np.random.Generator, **ranges):
    """`affine_samples` for polygon labels, as `augment_samples_seg` is to `augment_samples`: the same draws (the same seed gives the same
    `imgs`, bit for bit), `warp_batch` without masks, the vertices moved exactly on the host (`affine_polygons`) and rasterised at the
    canvas resolution, so nothing is resampled and the boxes of the rotated polygons stay tight.  Returns (imgs, masks, gt_rows, inst) as
    `augment_samples_seg` does; copy_paste=dict(...) as there.  Nothing synchronises with the host."""
    clahe, copy_paste = ranges.pop("clahe", None), ranges.pop("copy_paste", None)
    geo, pho, lab = _split(ranges, "affine_samples_seg", _AFFINE_KEYS)
    if len(seg_rows_per_image) != len(images):
        raise ValueError("affine_samples_seg: one list of label rows per image")
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    coef = affine_coefficients(sample_affine(sizes, img_size, rng, **geo))
    forward = affine_forward(coef)
    lut = _upload(torch.from_numpy(sample_photometric(len(images), rng, **pho)), images[0].device)
    imgs, _ = warp_batch(_equalised(images, rng, clahe), None, coef, lut, img_size)
    whole = (0, 0, int(img_size), int(img_size))
    per_canvas = [[(row6, v, whole) for row6, v in affine_polygons(r, W0, H0, forward[i], img_size, **lab)]
                  for i, (r, (H0, W0)) in enumerate(zip(seg_rows_per_image, sizes))]
    return _pasted((imgs,) + _seg_outputs(per_canvas, [[whole]] * len(images), img_size, imgs.device), per_canvas, img_size, rng, copy_paste)


# ---- copy-paste of instances between the canvases of a batch (the project's own definition: include/mtbt_hip.h `mtbt_copy_paste`) ----
PASTE_FIELDS = 8  # src_row, dx, dy, flip, 4 reserved zeros


def copy_paste_batch(imgs: torch.Tensor, planes: torch.Tensor, row_off, gt_rows: torch.Tensor, table, *, masks: bool = True):
    """Lay instances of the batch's canvases on its canvases.  imgs f32 [B,3,S,S], planes uint8 [M,S,pitch] (bit-packed, pitch =
    8 ceil(S / 64), row for row with gt_rows f32 [M,6]) -- all three CUDA tensors, what a `*_samples_seg` function returns -- row_off int
    [B + 1] on the HOST (canvas i owns the rows row_off[i] .. row_off[i + 1] - 1) and table = (paste_off int [B + 1], entries int [P, 8]) as
    `sample_copy_paste` returns it: entry rows (src_row, dx, dy, flip, 0, 0, 0, 0) grouped by destination canvas, at most 16 per canvas,
    later above earlier.  The rule is stated in include/mtbt_hip.h `mtbt_copy_paste`: the donor's pixels under its plane, mirrored first if
    flip, then moved by (dx, dy); exact copies; covered parts of older planes removed; boxes tight around what stays visible.
    Returns (imgs [B,3,S,S], masks [B,1,S,S] f32 {0,1} -- the union of each canvas's planes -- or None, gt_rows [M + P, 6], inst): the M old
    rows first, then the P pasted ones in table order; inst = dict(planes uint8 [M+P,S,pitch], image int64 [M+P], labels int64 [M+P],
    area int32 [M+P] visible pixels, area_before int32 [M+P] pixels before this call's layering, boxes int32 [M+P,4] x1 y1 x2 y2 with
    exclusive maxima).  A row that later pastes cover completely stays, as (image, cls, 0, 0, 0, 0): `loss.group_gt_rows_cls` skips it.
    The inputs are not modified.  One launch per <= 8 canvases plus a small one, no host synchronisation, no CPU path."""
    lib = L.load()
    for t, what in ((imgs, "imgs"), (planes, "planes"), (gt_rows, "gt_rows")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"copy_paste_batch: {what} must be a CUDA/HIP tensor on an MI355X (no CPU path)")
    if imgs.dtype != torch.float32 or imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[2] != imgs.shape[3]:
        raise ValueError("copy_paste_batch: imgs must be float32 [B, 3, S, S]")
    B, S = int(imgs.shape[0]), int(imgs.shape[3])
    pitch = plane_pitch(S)
    if planes.dtype != torch.uint8 or planes.dim() != 3 or tuple(planes.shape[1:]) != (S, pitch):
        raise ValueError(f"copy_paste_batch: planes must be uint8 [M, {S}, {pitch}]")
    M = int(planes.shape[0])
    if gt_rows.dtype != torch.float32 or tuple(gt_rows.shape) != (M, 6):
        raise ValueError(f"copy_paste_batch: gt_rows must be float32 [{M}, 6], one row per plane")
    ro = _int_array(row_off, (B + 1,), "copy_paste_batch", "row_off")
    po = _int_array(table[0], (B + 1,), "copy_paste_batch", "table[0] (paste_off)")
    ent = _int_array(np.asarray(table[1]).reshape(-1, PASTE_FIELDS), (None, PASTE_FIELDS), "copy_paste_batch", "table[1] (entries)")
    P = int(ent.shape[0])
    if ro[0] != 0 or po[0] != 0 or ro[-1] != M or po[-1] != P or (np.diff(ro) < 0).any() or (np.diff(po) < 0).any():
        raise ValueError("copy_paste_batch: row_off / paste_off must start at 0, not decrease, and end at the number of planes / entries")
    dev = imgs.device
    imgs, planes, gt_rows = imgs.contiguous(), planes.contiguous(), gt_rows.contiguous()
    N = M + P
    out = torch.empty_like(imgs)
    out_m = torch.empty(B, 1, S, S, device=dev, dtype=torch.float32) if masks else None
    out_planes = torch.empty(N, S, pitch, device=dev, dtype=torch.uint8)
    rows = torch.empty(N, 6, device=dev, dtype=torch.float32)
    area_before, area = torch.empty(N, device=dev, dtype=torch.int32), torch.empty(N, device=dev, dtype=torch.int32)
    boxes = torch.empty(N, 4, device=dev, dtype=torch.int32)
    a = L.CopyPasteArgs()
    a.images, a.planes, a.rows_in = imgs.data_ptr(), planes.data_ptr(), gt_rows.data_ptr()
    a.row_off, a.paste_off, a.entries = ro.ctypes.data_as(_INT32_P), po.ctypes.data_as(_INT32_P), ent.ctypes.data_as(_INT32_P)
    a.out_images, a.out_planes, a.out_masks, a.rows_out = out.data_ptr(), out_planes.data_ptr(), out_m.data_ptr() if masks else None, rows.data_ptr()
    a.area_before, a.area, a.box = area_before.data_ptr(), area.data_ptr(), boxes.data_ptr()
    a.B, a.M, a.P, a.S, a.pitch, a.entry_stride = B, M, P, S, pitch, PASTE_FIELDS
    stream = torch.cuda.current_stream(dev)
    L.check(lib.mtbt_copy_paste(C.byref(a), C.c_void_p(stream.cuda_stream)), "mtbt_copy_paste")
    for t in (imgs, planes, gt_rows):   # the launches are asynchronous: keep the inputs alive until the stream has consumed them
        t.record_stream(stream)
    image = np.concatenate([np.repeat(np.arange(B, dtype=np.int64), np.diff(ro)), np.repeat(np.arange(B, dtype=np.int64), np.diff(po))])
    inst = {"planes": out_planes, "image": _upload(torch.from_numpy(image), dev), "labels": rows[:, 1].to(torch.int64),
            "area": area, "area_before": area_before, "boxes": boxes}
    return out, out_m, rows, inst


def _box_px(row6, S: float):
    """A label row (image, cls, xc, yc, w, h), normalised -> (x1, y1, x2, y2) in canvas pixels, Python floats."""
    xc, yc, w, h = (float(v) * S for v in row6[2:6])
    return xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2


def sample_copy_paste(boxes_per_canvas: Sequence[Sequence[Sequence[float]]], img_size: int, rng: np.random.Generator, *, prob: float = 0.5,
                      fraction: float = 0.5, mode: str = "mix", translate: float = 0.0, max_ioa: float = 0.3, min_px: float = 2.0,
                      max_per_canvas: int = 16):
    """Draw the table of `copy_paste_batch` from the HOST-side label rows of the canvases, so nothing is read back from the device.
    boxes_per_canvas: per canvas its rows (image, cls, xc, yc, w, h), normalised to the canvas, in the order of the planes; the donor row of
    an entry is the row's index in the concatenation of all canvases.  Returns (paste_off int32 [B + 1], entries int32 [P, 8]).
    A canvas receives pastes with probability prob.  mode "mix": its donor is one OTHER canvas drawn uniformly (none when B == 1), mirrored
    with probability 0.5 and moved by integer offsets drawn uniformly from [-t, t], t = int(translate * S), per axis -- one donor, one flip
    and one offset per receiving canvas, so the donor's instances keep their arrangement.  mode "flip" is the classic form: the donor is the
    canvas itself, mirrored, not moved.  Every donor row, in row order, is a candidate with probability fraction; its box is mirrored
    (x -> S - x) and moved like the pixels, then clipped to the canvas; it is rejected when a clipped side is below min_px, or when
    inter(t, b) / area(b) >= max_ioa for any box b already on the canvas -- the canvas's own rows and the pastes accepted before it
    (ultralytics' test, on boxes: it needs no plane).  At most max_per_canvas (<= 16) entries per canvas.  Donor boxes are always those of
    the INPUT rows, as the pasted pixels are the input's.
    The draws come in a fixed order whatever the mode -- the decisions (B), the donors (B, integers below max(B - 1, 1); a value >= the
    canvas's own index names the next canvas), the flips (B), the offsets (B x 2: x, y; integers in [-t, t]), then, for each receiving
    canvas with a donor in canvas order, one vector of the donor's row count for the candidates -- so a seeded generator gives the same
    table again.  In mode "flip" the donor, flip and offset draws are made and not used."""
    if mode not in ("mix", "flip"):
        raise ValueError("sample_copy_paste: mode must be 'mix' or 'flip'")
    if not 0 <= int(max_per_canvas) <= L.COPY_PASTE_MAX_ENTRIES:
        raise ValueError(f"sample_copy_paste: max_per_canvas must lie in [0, {L.COPY_PASTE_MAX_ENTRIES}]")
    B, S = len(boxes_per_canvas), float(img_size)
    t = int(translate * S)
    if not 0 <= t <= int(img_size):
        raise ValueError("sample_copy_paste: translate must lie in [0, 1]")
    on = rng.random(B) < prob
    donors = rng.integers(0, max(B - 1, 1), B)
    flips = rng.random(B) < 0.5
    offsets = rng.integers(-t, t + 1, (B, 2))
    first_row = np.concatenate([[0], np.cumsum([len(c) for c in boxes_per_canvas])]).astype(np.int64)
    paste_off, entries = np.zeros(B + 1, dtype=np.int32), []
    for i in range(B):
        paste_off[i + 1] = paste_off[i]
        if not on[i] or (mode == "mix" and B == 1):
            continue
        if mode == "mix":
            j = int(donors[i]) + (int(donors[i]) >= i)
            flip, dx, dy = int(flips[i]), int(offsets[i, 0]), int(offsets[i, 1])
        else:
            j, flip, dx, dy = i, 1, 0, 0
        cand = rng.random(len(boxes_per_canvas[j])) < fraction
        placed = [_box_px(r, S) for r in boxes_per_canvas[i]]
        for k, r in enumerate(boxes_per_canvas[j]):
            if paste_off[i + 1] - paste_off[i] >= max_per_canvas:
                break
            if not cand[k]:
                continue
            x1, y1, x2, y2 = _box_px(r, S)
            if flip:
                x1, x2 = S - x2, S - x1
            x1, y1, x2, y2 = (min(max(v, 0.0), S) for v in (x1 + dx, y1 + dy, x2 + dx, y2 + dy))
            if x2 - x1 < min_px or y2 - y1 < min_px:
                continue
            if any(_ioa((x1, y1, x2, y2), b) >= max_ioa for b in placed):
                continue
            placed.append((x1, y1, x2, y2))
            entries.append([int(first_row[j]) + k, dx, dy, flip, 0, 0, 0, 0])
            paste_off[i + 1] += 1
    return paste_off, np.asarray(entries, dtype=np.int32).reshape(-1, PASTE_FIELDS)


def _ioa(t, b) -> float:
    """inter(t, b) / area(b) of two (x1, y1, x2, y2) boxes; 0 for a box b without area."""
    area = (b[2] - b[0]) * (b[3] - b[1])
    if not area > 0.0:
        return 0.0
    return max(min(t[2], b[2]) - max(t[0], b[0]), 0.0) * max(min(t[3], b[3]) - max(t[1], b[1]), 0.0) / area


def _pasted(outputs, per_canvas, img_size: int, rng: np.random.Generator, copy_paste: Optional[dict]):
    """The `copy_paste=dict(...)` option of the `*_samples_seg` functions: outputs = (imgs, masks, gt_rows, inst) of the canvases as drawn,
    per_canvas their host-side items (label row first).  None draws nothing and returns the outputs; otherwise `sample_copy_paste` on the
    label rows -- the last draws of the call -- then `copy_paste_batch`."""
    if copy_paste is None:
        return outputs
    imgs, _, gt_rows, inst = outputs
    row_off = np.concatenate([[0], np.cumsum([len(c) for c in per_canvas])]).astype(np.int32)
    table = sample_copy_paste([[it[0] for it in c] for c in per_canvas], img_size, rng, **copy_paste)
    return copy_paste_batch(imgs, inst["planes"], row_off, gt_rows, table)


# ---- sliced inference: overlapping tiles of a large image (the project's own definition: include/mtbt_hip.h `mtbt_tile`) ----
def _axis_origins(L: int, S: int, overlap: float, up: int) -> List[int]:
    """Tile origins along an axis of resized length L: one at 0 if L <= S, else ceil((L - S overlap) / (S (1 - overlap))) spread evenly
    from 0 to L - S, each rounded down to a multiple of `up`, the last one rounded up (the end is covered, the overhang is pad)."""
    if L <= S:
        return [0]
    n = max(2, math.ceil((L - S * overlap) / (S * (1.0 - overlap))))
    out = [int(i * (L - S) / (n - 1)) // up * up for i in range(n - 1)]
    return out + [-(-(L - S) // up) * up]


def _window(o: int, S: int, new: int, z: float, extent: int):
    """The frame pixels X whose centre (X + 0.5) z lies in [o, min(o + S, new)), half-open, clamped to the image; the tile that reaches the
    end of the resized axis takes the pixels up to the image's edge (int(extent z) may cut the last centre off)."""
    lo = max(0, math.ceil(o / z - 0.5))
    hi = extent if o + S >= new else min(extent, math.ceil(min(o + S, new) / z - 0.5))
    return lo, max(hi, lo)


def _tile(image: int, H0: int, W0: int, z: float, ox: int, oy: int, S: int, up: int) -> dict:
    new_w, new_h = max(1, int(W0 * z)), max(1, int(H0 * z))
    wx0, wx1 = _window(ox, S, new_w, z, W0)
    wy0, wy1 = _window(oy, S, new_h, z, H0)
    return {"image": image, "pox": ox // up, "poy": oy // up, "wx0": wx0, "wy0": wy0, "wx1": wx1, "wy1": wy1, "height": H0, "width": W0,
            "step": C.c_float(z / up).value, "scale": C.c_float(z).value, "fox": float(ox), "foy": float(oy), "zoom": z, "ox": ox, "oy": oy,
            "geom": [new_w, new_h, -ox, -oy, 0, 0, 0, 0]}


def slice_geometry(sizes: Sequence[Sequence[int]], img_size: int, zoom: float = 1.0, overlap: float = 0.2, full_view: bool = True,
                   up: int = 4) -> List[List[dict]]:
    """The tiles of sliced inference.  sizes: (H0, W0) per image.  A pass at `zoom` resizes the image by the letterbox's rule
    (new = max(1, int(dim * zoom)); never materialised) and cuts it into S x S tiles (S = img_size) that overlap by about `overlap` of
    S, row-major, origins multiples of `up` (letterboxed pixels per prototype pixel, S / G); with `full_view` the whole image at
    S / max(H0, W0) -- the plain letterbox -- comes last, unless the pass is one tile already.  Returns per image the list of its tiles:
    dicts of the `mtbt_tile` fields (image, pox, poy, window wx0 wy0 wx1 wy1 half-open in image pixels, height, width, step =
    float32(zoom / up) which must lie in (0, 1], scale = float32(zoom), fox, foy) plus `geom`, the `augment_batch` row (new_w, new_h,
    -ox, -oy, 0, 0, 0, 0) that draws the tile, and zoom / ox / oy."""
    S, up = int(img_size), int(up)
    if not 0.0 <= overlap < 1.0 or zoom <= 0 or S % up:
        raise ValueError(f"slice_geometry: overlap {overlap} (0 <= overlap < 1), zoom {zoom} (> 0), img_size {S} (a multiple of up = {up})")
    out = []
    for n, (H0, W0) in enumerate(sizes):
        H0, W0 = int(H0), int(W0)
        new_w, new_h = max(1, int(W0 * zoom)), max(1, int(H0 * zoom))
        tiles = [_tile(n, H0, W0, float(zoom), ox, oy, S, up) for oy in _axis_origins(new_h, S, overlap, up) for ox in _axis_origins(new_w, S, overlap, up)]
        if full_view and len(tiles) > 1:
            tiles.append(_tile(n, H0, W0, S / max(H0, W0), 0, 0, S, up))
        for t in tiles:
            if not 0.0 < t["step"] <= 1.0:
                raise ValueError(f"slice_geometry: image {n} ({H0} x {W0}) at zoom {t['zoom']} gives {t['step']} prototype pixels per image pixel; "
                                 "the supported range is 0 < zoom / up <= 1")
        if len(tiles) > 64:
            raise ValueError(f"slice_geometry: image {n} ({H0} x {W0}) needs {len(tiles)} tiles (64 at most): lower zoom or raise img_size")
        out.append(tiles)
    return out


def slice_batch(images: Sequence[torch.Tensor], tiles: Sequence[Sequence[dict]], img_size: int = 640) -> torch.Tensor:
    """The canvases of `slice_geometry`'s tiles, [NT,3,S,S] f32 RGB in [0,1], tile-major in the order of `tiles`: `augment_batch` with each
    tile's geometry row and its image's descriptor repeated (no new pixel kernel, no table)."""
    if len(tiles) != len(images):
        raise ValueError(f"slice_batch: {len(tiles)} tile lists for {len(images)} images")
    flat = [t for per in tiles for t in per]
    geom = np.asarray([t["geom"] for t in flat], dtype=np.int32).reshape(len(flat), GEOM_FIELDS)
    return augment_batch([images[t["image"]] for t in flat], None, geom, None, img_size)[0]
