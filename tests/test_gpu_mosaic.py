"""HIP four-image mosaic (mtbt_mosaic_batch) against tests/mosaic_reference.py and against the device's own `augment_batch`: bit-exact,
as the augmentation is (integer arithmetic past the coefficient set-up, a byte lookup, one correctly rounded fp32 division).  The
arithmetic is the project's own definition (include/mtbt_hip.h)."""
import functools

import numpy as np
import pytest
import torch

from augment_reference import augment
from mosaic_reference import mosaic, rectangles

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64
SOURCES = [(1, 5), (5, 1), (2, 2), (64, 63), (129, 127), (37, 91)]
CENTRES = [(0, 0), (64, 64), (0, 64), (64, 0), (32, 32), (4, 1), (60, 63), (32, 17)]


def _sample(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def _row(kind, orient, rect):
    """A geometry row for a tile with rectangle rect, in canvas coordinates."""
    x0, y0, x1, y1 = rect
    big = int(2.3 * S)
    nw, nh = [(S - 20, S - 30), (big, big), (big, S - 30), (S - 1, big), (1, 1), (S, S), (S - 24, 1), (S - 20, S - 30), (big, big)][kind]
    qw, qh = (nh, nw) if orient & 4 else (nw, nh)
    ox, oy = [((x0 if x0 else x1 - qw), (y0 if y0 else y1 - qh)),   # the corner facing the centre touches it
              (x0 - 10, y0 - 7),                                     # larger than the tile, cropped on every side (negative for tile 0)
              (x0 - qw // 2, y1 - 1),                                # one visible row, at the tile's last row
              (x1 - 1, y0 - qh // 2),                                # one visible column, at the tile's last column
              (x1 - 1, y1 - 1),                                      # one pixel in the tile's far corner
              (0, 0),                                                # the whole canvas: the tile is a window on it
              (x0 + 3, y0 + 2),
              ((x1 if x0 == 0 else x0 - qw), y0),                    # wholly outside the tile, inside a neighbour's rectangle
              (-100000, y0)][kind]                                   # wholly outside the canvas
    return [nw, nh, ox, oy, orient, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def _canvases():
    """Every centre x every orientation; the four tiles of a canvas take different sources, orientations and kinds of row, and over
    the canvases every tile position meets every kind.  Returns (images, masks, index, geom, centres, lut) in numpy."""
    imgs, masks = zip(*[_sample(h, w, seed=h * 131 + w) for h, w in SOURCES])
    index, geom, centres = [], [], []
    for ci, centre in enumerate(CENTRES):
        rects = rectangles(centre, S)
        for orient in range(8):
            n = len(index)
            index.append([(n + t) % len(SOURCES) for t in range(4)])
            geom.append([_row((n + 2 * t + ci) % 9, (orient + 3 * t) % 8, rects[t]) for t in range(4)])
            centres.append(centre)
    index, geom, centres = np.array(index), np.array(geom, dtype=np.int32), np.array(centres, dtype=np.int32)
    lut = np.random.default_rng(7).integers(0, 256, size=(len(index), 3, 256), dtype=np.uint8)
    return list(imgs), list(masks), index, geom, centres, lut


def _device(arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@pytest.mark.parametrize("table", [False, True])
def test_mosaic_matches_reference(table):
    from multitask_bonetumor_yolo_amd import preprocess as P
    imgs, masks, index, geom, centres, lut = _canvases()
    assert set(geom[:, :, 4].reshape(-1).tolist()) == set(range(8))
    x, m = P.mosaic_batch(_device(imgs), _device(masks), index, geom, centres, torch.from_numpy(lut).to(DEV) if table else None, S)
    torch.cuda.synchronize()
    n = len(index)
    assert x.shape == (n, 3, S, S) and m.shape == (n, 1, S, S) and x.dtype == m.dtype == torch.float32
    x, m = x.cpu().numpy(), m.cpu().numpy()
    for i in range(n):
        rx, rm = mosaic([imgs[k] for k in index[i]], [masks[k] for k in index[i]], geom[i], centres[i], S, lut=lut[i] if table else None)
        assert np.array_equal(x[i], rx) and np.array_equal(m[i], rm), f"canvas {i} centre {centres[i].tolist()} index {index[i].tolist()} geom {geom[i].tolist()}"


def test_mosaic_is_four_augment_batches_cut_at_the_centre():
    from multitask_bonetumor_yolo_amd import preprocess as P
    imgs, masks, index, geom, centres, lut = _canvases()
    di, dm, dl = _device(imgs), _device(masks), torch.from_numpy(lut).to(DEV)
    x, m = P.mosaic_batch(di, dm, index, geom, centres, dl, S)
    n = len(index)
    xs = torch.arange(S, device=DEV).view(1, 1, 1, S)
    ys = torch.arange(S, device=DEV).view(1, 1, S, 1)
    cx, cy = (torch.from_numpy(centres[:, k].astype(np.int64)).to(DEV).view(n, 1, 1, 1) for k in (0, 1))
    tile = (xs >= cx).long() + 2 * (ys >= cy).long()                                   # [n, 1, S, S]: which tile owns the pixel
    wx, wm = torch.full_like(x, -1.0), torch.full_like(m, -1.0)
    for t in range(4):
        ax, am = P.augment_batch([di[k] for k in index[:, t]], [dm[k] for k in index[:, t]], geom[:, t], dl, S)
        wx, wm = torch.where(tile == t, ax, wx), torch.where(tile == t, am, wm)
    torch.cuda.synchronize()
    assert torch.equal(x, wx) and torch.equal(m, wm)


@pytest.mark.parametrize("size,sizes", [(64, SOURCES), (640, [(480, 640), (1000, 700)])])
def test_degenerate_centre_is_augment_batch(size, sizes):
    from multitask_bonetumor_yolo_amd import preprocess as P
    imgs, masks = zip(*[_sample(h, w, i) for i, (h, w) in enumerate(sizes)])
    di, dm = _device(imgs), _device(masks)
    n = len(sizes)
    rng = np.random.default_rng(size)
    geom = P.sample_geometry([sizes[k % n] for k in range(4 * n)], size, rng, scale=(0.5, 1.6), aspect=0.2, fliplr=0.5, flipud=0.5, transpose=0.5).reshape(n, 4, 8)
    index = np.array([[(i + t) % n for t in range(4)] for i in range(n)])
    geom[:, 0] = P.sample_geometry(sizes, size, rng, scale=(0.5, 1.6), aspect=0.2, fliplr=0.5, flipud=0.5, transpose=0.5)
    lut = torch.from_numpy(P.sample_photometric(n, rng)).to(DEV)
    centres = np.full((n, 2), size, dtype=np.int32)
    for table in (None, lut):
        x, m = P.mosaic_batch(di, dm, index, geom, centres, table, size)
        ax, am = P.augment_batch(di, dm, geom[:, 0], table, size)
        torch.cuda.synchronize()
        assert torch.equal(x, ax) and torch.equal(m, am)


def test_mosaic_many_canvases_strided_rows_missing_masks_and_shared_sources():
    from multitask_bonetumor_yolo_amd import preprocess as P
    size, n = 32, 11                                                                   # 11 canvases: two launch chunks of <= 8
    wide = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(40, 90, 3), dtype=np.uint8)).to(DEV)
    imgs = [wide[:, 10 * (i % 5): 10 * (i % 5) + 20 + i] for i in range(n)]          # views with a 270-byte row stride
    masks = [None if i % 2 else (wide[:, :, 0] > 99).to(torch.uint8)[:, 10 * (i % 5): 10 * (i % 5) + 20 + i] * 255 for i in range(n)]
    rng = np.random.default_rng(4)
    index, geom, centres = P.sample_mosaic([tuple(a.shape[:2]) for a in imgs], size, rng, scale=(0.4, 2.5), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)
    index[3] = 6                                                                       # one source in all four tiles of a canvas
    index[9, 1:] = index[9, 0]
    lut = P.sample_photometric(n, rng)
    x, m = P.mosaic_batch(imgs, masks, index, geom, centres, torch.from_numpy(lut).to(DEV), size)
    torch.cuda.synchronize()
    assert len(set(index.reshape(-1).tolist())) > 6 and any(masks[k] is None for k in index[8:].reshape(-1)) and m.any()
    host_i = [a.cpu().numpy() for a in imgs]
    host_m = [None if a is None else a.cpu().numpy() for a in masks]
    for i in range(n):
        rx, rm = mosaic([host_i[k] for k in index[i]], [host_m[k] for k in index[i]], geom[i], centres[i], size, lut=lut[i])
        assert np.array_equal(x[i].cpu().numpy(), rx) and np.array_equal(m[i].cpu().numpy(), rm), (i, centres[i].tolist(), geom[i].tolist())


ROWS = [[[1, 0.5, 0.5, 0.6, 0.6], [0, 0.3, 0.4, 0.3, 0.5]], [], [[0, 0.5, 0.5, 0.9, 0.9]], [[1, 0.4, 0.6, 0.5, 0.7]]]
SIZES = [(90, 60), (50, 120), (64, 64), (33, 47)]


def test_mosaic_samples_output_contract():
    import multitask_bonetumor_yolo_amd as pkg
    imgs, masks = zip(*[_sample(h, w, i) for i, (h, w) in enumerate(SIZES)])
    di, dm = _device(imgs), _device(masks)
    kw = dict(scale=(0.6, 1.0), aspect=0.1, flipud=0.5, transpose=0.5, prob=0.75)
    x, m, gt = pkg.mosaic_samples(di, dm, ROWS, S, np.random.default_rng(21), **kw)
    x2, m2, gt2 = pkg.mosaic_samples(di, dm, ROWS, S, np.random.default_rng(21), **kw)
    torch.cuda.synchronize()
    for t, shape in ((x, (4, 3, S, S)), (m, (4, 1, S, S))):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    assert gt.is_cuda and gt.dtype == torch.float32 and gt.dim() == 2 and gt.shape[1] == 6 and gt.shape[0] >= 1
    assert set(gt[:, 0].tolist()) <= {0.0, 1.0, 2.0, 3.0} and set(gt[:, 1].tolist()) <= {0.0, 1.0}
    assert bool(((gt[:, 2:] >= 0) & (gt[:, 2:] <= 1)).all()) and bool((gt[:, 4:] > 0).all())
    assert torch.equal(x, x2) and torch.equal(m, m2) and torch.equal(gt, gt2)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0 and set(m.unique().tolist()) <= {0.0, 1.0}
    # the same draws by hand: the mosaic, then the tables, from one generator
    rng = np.random.default_rng(21)
    geo = {k: v for k, v in kw.items()}
    index, geom, centres = pkg.sample_mosaic(SIZES, S, rng, **geo)
    lut = pkg.sample_photometric(4, rng)
    hx, hm = pkg.mosaic_batch(di, dm, index, geom, centres, torch.from_numpy(lut).to(DEV), S)
    assert torch.equal(x, hx) and torch.equal(m, hm)
    for i in range(4):
        rx, rm = mosaic([imgs[k] for k in index[i]], [masks[k] for k in index[i]], geom[i], centres[i], S, lut=lut[i])
        assert np.array_equal(x[i].cpu().numpy(), rx) and np.array_equal(m[i].cpu().numpy(), rm)
    want = pkg.preprocess.collate_boxes([pkg.mosaic_yolo_labels([ROWS[k] for k in index[i]], [SIZES[k] for k in index[i]], geom[i], centres[i], S)
                                         for i in range(4)])
    assert torch.equal(gt.cpu(), want)
    with pytest.raises(TypeError):
        pkg.mosaic_samples(di, dm, ROWS, S, np.random.default_rng(0), place="random")
    with pytest.raises(ValueError):
        pkg.mosaic_samples(di, dm, ROWS[:3], S, np.random.default_rng(0))


def test_without_mosaic_the_samples_are_augment_batch_of_tile_0():
    import multitask_bonetumor_yolo_amd as pkg
    imgs, masks = zip(*[_sample(h, w, i) for i, (h, w) in enumerate(SIZES)])
    di, dm = _device(imgs), _device(masks)
    kw = dict(scale=(0.6, 1.4), aspect=0.1, flipud=0.5, transpose=0.5, prob=0.0)
    x, m, gt = pkg.mosaic_samples(di, dm, ROWS, S, np.random.default_rng(33), **kw)
    rng = np.random.default_rng(33)                                                    # the same generator state
    index, geom, centres = pkg.sample_mosaic(SIZES, S, rng, **kw)
    lut = torch.from_numpy(pkg.sample_photometric(4, rng)).to(DEV)
    assert np.all(centres == S) and np.array_equal(index[:, 0], np.arange(4))
    ax, am = pkg.augment_batch(di, dm, geom[:, 0], lut, S)
    torch.cuda.synchronize()
    assert torch.equal(x, ax) and torch.equal(m, am)
    want = pkg.preprocess.collate_boxes([pkg.augment_yolo_labels(r, W0, H0, geom[i, 0], S) for i, (r, (H0, W0)) in enumerate(zip(ROWS, SIZES))])
    assert torch.equal(gt.cpu(), want)


def test_mosaic_rejects_bad_input():
    from multitask_bonetumor_yolo_amd import preprocess as P
    index = np.zeros((1, 4), dtype=np.int64)
    geom = np.tile(np.array([4, 4, 0, 0, 0, 0, 0, 0], dtype=np.int32), (1, 4, 1))
    centres = np.array([[32, 17]], dtype=np.int32)
    ok = torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV)
    x, m = P.mosaic_batch([ok], None, index, geom, centres, None, 64)                              # the good call
    assert x.shape == (1, 3, 64, 64) and not m.any()
    with pytest.raises(RuntimeError):
        P.mosaic_batch([torch.zeros(4, 4, 3, dtype=torch.uint8)], None, index, geom, centres, None, 64)   # CPU tensor: no CPU path
    with pytest.raises(ValueError):
        P.mosaic_batch([torch.zeros(4, 4, 3, device=DEV)], None, index, geom, centres, None, 64)   # not uint8
    for bad in (np.array([[0, 0, 1, 0]]), np.array([[0, -1, 0, 0]])):
        with pytest.raises(ValueError):
            P.mosaic_batch([ok], None, bad, geom, centres, None, 64)                               # index out of range
    with pytest.raises(RuntimeError):
        P.mosaic_batch([ok], None, index, geom, np.array([[30, 17]], dtype=np.int32), None, 64)    # cx % 4
    with pytest.raises(RuntimeError):
        P.mosaic_batch([ok], None, index, geom, np.array([[32, 65]], dtype=np.int32), None, 64)    # cy beyond S
    with pytest.raises(RuntimeError):
        P.mosaic_batch([ok], None, index, geom, centres, None, 62)                                 # S % 4
    worse = geom.copy()
    worse[0, 3, 4] = 8
    with pytest.raises(RuntimeError):
        P.mosaic_batch([ok], None, index, worse, np.array([[64, 64]], dtype=np.int32), None, 64)   # orient = 8 in an empty tile
    for args in ((index[:, :3], geom, centres), (index, geom[:, :3], centres), (index, geom[:, :, :7], centres), (index, geom[0], centres),
                 (index, geom, centres[:, :1]), (index, geom, np.tile(centres, (2, 1))), (index.astype(np.float32), geom, centres),
                 (index, geom.astype(np.float32), centres), (index, geom, centres.astype(np.float64))):
        with pytest.raises(ValueError):
            P.mosaic_batch([ok], None, *args, None, 64)                                            # wrong shapes / not integers
    with pytest.raises(ValueError):
        P.mosaic_batch([ok], None, index, geom, centres, torch.zeros(1, 3, 256, dtype=torch.uint8), 64)   # table on the host
