"""The CLAHE rule of include/mtbt_hip.h (`mtbt_clahe_batch`) restated in numpy: the reference of tests/test_gpu_clahe.py, itself checked
against a scalar form and a float64 form in cv2's terms by tests/test_cpu_clahe.py.  Vectorised: a 2048 x 1536 image takes a fraction of
a second.  Images are uint8 [H, W] or [H, W, 3]; the grid is (gx, gy); clip is the INTEGER of the rule (`preprocess.clahe_clip`)."""
import numpy as np


def tile_size(H: int, W: int, grid):
    gx, gy = int(grid[0]), int(grid[1])
    return -(-int(W) // gx), -(-int(H) // gy)


def keys(img: np.ndarray) -> np.ndarray:
    """The key plane [H, W] (int64) the curves are built from."""
    v = img.astype(np.int64)
    return v if v.ndim == 2 else (v[..., 0] + 2 * v[..., 1] + v[..., 2] + 2) >> 2


def _reflect(n_ext: int, n: int) -> np.ndarray:
    i = np.arange(n_ext)
    return np.where(i < n, i, 2 * (n - 1) - i)


def tile_hists(img: np.ndarray, grid) -> np.ndarray:
    """int64 [gy, gx, 256]: the key counts of every tile of the reflect-extended image."""
    gx, gy = int(grid[0]), int(grid[1])
    H, W = img.shape[:2]
    tw, th = tile_size(H, W, grid)
    k = keys(img)[_reflect(gy * th, H)][:, _reflect(gx * tw, W)]
    tile = (np.arange(gy * th) // th)[:, None] * gx + (np.arange(gx * tw) // tw)[None, :]
    return np.bincount((tile * 256 + k).ravel(), minlength=gx * gy * 256).reshape(gy, gx, 256)


def clip_hists(hist: np.ndarray, clip: int) -> np.ndarray:
    """The clip step on int64 [..., 256] histograms (closed form of the remainder); clip == 0 returns them unchanged."""
    hist = hist.astype(np.int64)
    if clip <= 0:
        return hist
    excess = np.maximum(hist - clip, 0).sum(axis=-1)
    out = np.minimum(hist, clip) + (excess // 256)[..., None]
    r = excess % 256
    step = np.maximum(256 // np.maximum(r, 1), 1)
    b = np.arange(256)
    return out + ((b % step[..., None] == 0) & (b // step[..., None] < r[..., None]))


def curves(hist: np.ndarray, area: int) -> np.ndarray:
    """int64 [..., 256] histograms that sum to area -> the rounded curves, int64 [..., 256]."""
    return (510 * np.cumsum(hist, axis=-1) + area) // (2 * area)


def tile_luts(img: np.ndarray, grid, clip: int) -> np.ndarray:
    """int64 [gy, gx, 256]."""
    tw, th = tile_size(img.shape[0], img.shape[1], grid)
    return curves(clip_hists(tile_hists(img, grid), int(clip)), tw * th)


def _axis(n: int, t: int, g: int):
    """Per index of an axis: (first tile, second tile, weight of the first, weight of the second)."""
    u = 2 * np.arange(n) + 1 - t
    t1 = u // (2 * t)                     # floor, -1 in the first half tile
    a = u - t1 * 2 * t
    return np.clip(t1, 0, g - 1), np.clip(t1 + 1, 0, g - 1), 2 * t - a, a


def interpolate(img: np.ndarray, luts: np.ndarray, grid) -> np.ndarray:
    gx, gy = int(grid[0]), int(grid[1])
    H, W = img.shape[:2]
    tw, th = tile_size(H, W, grid)
    x0, x1, wx0, wx1 = _axis(W, tw, gx)
    y0, y1, wy0, wy1 = _axis(H, th, gy)
    ex = (lambda a: a[..., None]) if img.ndim == 3 else (lambda a: a)
    v = img.astype(np.int64)
    total = np.zeros(img.shape, dtype=np.int64)
    for ty, wy in ((y0, wy0), (y1, wy1)):
        for tx, wx in ((x0, wx0), (x1, wx1)):
            total += ex(wy[:, None] * wx[None, :]) * luts[ex(ty[:, None]), ex(tx[None, :]), v]
    return ((total + 2 * tw * th) // (4 * tw * th)).astype(np.uint8)


def clahe(img: np.ndarray, grid, clip: int) -> np.ndarray:
    """The whole rule: uint8 image of the input's shape."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    return interpolate(img, tile_luts(img, grid, clip), grid)


def radiograph(rng: np.random.Generator, H: int, W: int, channels: int = 1) -> np.ndarray:
    """A radiograph-like test image: a large black background, a smooth bright body, fine noise inside it."""
    y, x = np.mgrid[0:H, 0:W]
    body = np.exp(-(((x - 0.55 * W) / (0.22 * W)) ** 2 + ((y - 0.5 * H) / (0.35 * H)) ** 2) * 2.0)
    v = 200.0 * body + 25.0 * np.sin(x / 7.0) * np.cos(y / 11.0) * body + rng.normal(0.0, 6.0, (H, W)) * (body > 0.05)
    g = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    g[body < 0.02] = 0
    if channels == 1:
        return g
    return np.ascontiguousarray(np.stack([g, np.clip(g.astype(np.int64) + rng.integers(-3, 4, (H, W)), 0, 255).astype(np.uint8), g], axis=-1))
