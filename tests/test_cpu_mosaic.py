"""Four-image mosaic without a GPU: the numpy restatement (tests/mosaic_reference.py) against the augmentation's, the host side of
`preprocess` (the seeded sampler, the label arithmetic per tile, pixel / label consistency) and the argument checks of
`mtbt_mosaic_batch`, which refuse a bad call before any launch.  The arithmetic is the project's own definition (include/mtbt_hip.h)."""
import ctypes as C

import numpy as np
import pytest

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import preprocess as P

from augment_reference import augment
from mosaic_reference import mosaic, rectangles

EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch
PAD = np.float32(114) / np.float32(255)


def _img(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def _four(S=32):
    sizes = [(20, 30), (41, 17), (32, 32), (9, 50)]
    imgs, masks = zip(*[_img(h, w, seed=i + 1) for i, (h, w) in enumerate(sizes)])
    geom = np.array([[40, 28, -5, -3, 1, 0, 0, 0], [25, 45, 3, -9, 4, 0, 0, 0], [32, 32, 0, 0, 2, 0, 0, 0], [50, 20, -12, 7, 7, 0, 0, 0]], dtype=np.int32)
    lut = np.random.default_rng(3).integers(0, 256, size=(3, 256), dtype=np.uint8)
    return list(imgs), list(masks), geom, lut


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_reference_at_the_degenerate_centre_is_augment():
    S = 32
    imgs, masks, geom, lut = _four(S)
    for table in (None, lut):
        x, m = mosaic(imgs, masks, geom, (S, S), S, lut=table)
        rx, rm = augment(imgs[0], masks[0], geom[0], S, lut=table)
        assert np.array_equal(x, rx) and np.array_equal(m, rm)


@pytest.mark.parametrize("centre,tile", [((0, 0), 3), ((32, 0), 2), ((0, 32), 1)])
def test_reference_shows_one_tile_alone_at_a_corner_centre(centre, tile):
    S = 32
    imgs, masks, geom, lut = _four(S)
    x, m = mosaic(imgs, masks, geom, centre, S, lut=lut)
    rx, rm = augment(imgs[tile], masks[tile], geom[tile], S, lut=lut)
    assert np.array_equal(x, rx) and np.array_equal(m, rm)


def test_reference_tiles_are_cut_at_the_centre():
    S = 32
    imgs, masks, geom, lut = _four(S)
    masks[1] = None                                                                   # a tile without a mask contributes zeros
    x, m = mosaic(imgs, masks, geom, (12, 21), S, lut=lut)
    for t, (x0, y0, x1, y1) in enumerate(rectangles((12, 21), S)):
        rx, rm = augment(imgs[t], masks[t], geom[t], S, lut=lut)
        assert np.array_equal(x[:, y0:y1, x0:x1], rx[:, y0:y1, x0:x1]) and np.array_equal(m[:, y0:y1, x0:x1], rm[:, y0:y1, x0:x1])
    assert not m[:, :21, 12:].any() and m.any()
    assert sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in rectangles((12, 21), S)) == S * S


# ---- sampling ------------------------------------------------------------------------------------------------------------------
KW = dict(scale=(0.5, 1.0), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)


def test_sample_mosaic_is_seeded_and_follows_the_corner_rule():
    S = 64
    sizes = [(90, 60), (50, 120), (7, 300), (64, 64)] * 100
    n = len(sizes)
    index, geom, centres = P.sample_mosaic(sizes, S, np.random.default_rng(11), centre=(0.25, 0.75), **KW)
    again = P.sample_mosaic(sizes, S, np.random.default_rng(11), centre=(0.25, 0.75), **KW)
    other = P.sample_mosaic(sizes, S, np.random.default_rng(12), centre=(0.25, 0.75), **KW)
    assert index.shape == (n, 4) and index.dtype.kind == "i" and geom.shape == (n, 4, 8) and geom.dtype == np.int32
    assert centres.shape == (n, 2) and centres.dtype == np.int32
    assert all(np.array_equal(a, b) for a, b in zip((index, geom, centres), again))
    assert not all(np.array_equal(a, b) for a, b in zip((index, geom, centres), other))
    assert not (centres[:, 0] % 4).any()
    assert centres.min() >= 16 and centres.max() <= 48                                # the band 0.25 S .. 0.75 S, floored
    assert len(np.unique(centres[:, 0])) > 4 and len(np.unique(centres[:, 1])) > 16
    assert index.min() >= 0 and index.max() < n
    own = (index == np.arange(n)[:, None])
    assert own.any(axis=1).all()                                                      # every canvas shows its own image ...
    first_own = own.argmax(axis=1)
    assert set(first_own.tolist()) == {0, 1, 2, 3}                                    # ... in a tile that varies
    assert len(np.unique(index[~own])) > n // 2                                       # the others come from the whole batch
    assert not geom[:, :, 5:].any() and set(np.unique(geom[:, :, 4])) == set(range(8))
    lo, hi = 0.5 * np.exp(-0.3), 1.0 * np.exp(0.3)
    for i in range(n):
        cx, cy = (int(v) for v in centres[i])
        for t in range(4):
            H0, W0 = sizes[index[i, t]]
            nw, nh, ox, oy, orient = geom[i, t, :5].tolist()
            s = S / max(H0, W0)
            assert max(1, int(W0 * s * lo)) <= nw <= max(1, int(W0 * s * hi) + 1) and max(1, int(H0 * s * lo)) <= nh <= max(1, int(H0 * s * hi) + 1)
            qw, qh = (nh, nw) if orient & 4 else (nw, nh)
            assert (ox, oy) == ((cx if t & 1 else cx - qw), (cy if t & 2 else cy - qh)), (i, t)   # the corner facing the centre touches it


def test_sample_mosaic_without_mosaic_is_the_plain_augmentation():
    S = 64
    sizes = [(90, 60), (50, 120), (7, 300), (64, 64)] * 10
    index, geom, centres = P.sample_mosaic(sizes, S, np.random.default_rng(5), prob=0.0, **KW)
    assert np.array_equal(index, np.repeat(np.arange(40)[:, None], 4, axis=1))
    assert np.all(centres == S)
    want = P.letterbox_geometry(sizes, S)
    for t in (1, 2, 3):
        assert np.array_equal(geom[:, t], want)
    for (H0, W0), (nw, nh, ox, oy, orient) in zip(sizes, geom[:, 0, :5].tolist()):   # a sample_geometry(place="random") row
        qw, qh = (nh, nw) if orient & 4 else (nw, nh)
        for off, q in ((ox, qw), (oy, qh)):
            assert min(0, S - q) <= off <= max(0, S - q)
    assert len(np.unique(geom[:, 0, 2])) > 5
    _, _, mixed = P.sample_mosaic(sizes * 10, S, np.random.default_rng(5), prob=0.5, **KW)
    plain = int(np.all(mixed == S, axis=1).sum())
    assert 120 < plain < 280                                                          # 400 canvases, each plain with probability 1/2


def test_sampled_rows_pass_the_entry_points_checks(lib):
    S = 64
    sizes = [(90, 60), (50, 120), (1, 3000), (64, 64), (3000, 2)] * 8
    index, geom, centres = P.sample_mosaic(sizes, S, np.random.default_rng(2), prob=0.7, scale=(0.01, 3.0), aspect=1.0, fliplr=0.5, flipud=0.5,
                                           transpose=0.5, centre=(0.0, 1.0))
    n = len(sizes)
    descs = (L.RawImage * (4 * n))()
    for d, k in zip(descs, index.reshape(-1)):
        H0, W0 = sizes[k]
        d.bgr, d.mask, d.height, d.width, d.row_stride, d.mask_row_stride = PTR, PTR, H0, W0, 3 * W0, W0
    g, c = np.ascontiguousarray(geom, np.int32), np.ascontiguousarray(centres, np.int32)
    # a misaligned output is refused only after every canvas passed its checks, and before any launch
    assert lib.mtbt_mosaic_batch(descs, n, S, g.ctypes.data_as(C.POINTER(C.c_int32)), 8, c.ctypes.data_as(C.POINTER(C.c_int32)), None, PTR + 4, PTR, None) == EALIGN


# ---- labels --------------------------------------------------------------------------------------------------------------------
def test_labels_of_a_box_that_straddles_the_centre_by_hand():
    # source 100 x 50, box x [20, 40], y [10, 30];  R is 40 x 30: x [8, 16], y [6, 18];  offsets (20, 10): canvas x [28, 36], y [16, 28]
    W0, H0, S = 100, 50, 64
    rows, g = [[1, 0.3, 0.4, 0.2, 0.4]], [40, 30, 20, 10, 0, 0, 0, 0]
    out = P.mosaic_yolo_labels([rows] * 4, [(H0, W0)] * 4, [g] * 4, (32, 20), S)
    want = [(30, 18, 4, 4),      # tile 0 [0,32) x [0,20): x [28, 32], y [16, 20]
            (34, 18, 4, 4),      # tile 1 [32,64) x [0,20): x [32, 36], y [16, 20]
            (30, 24, 4, 8),      # tile 2 [0,32) x [20,64): x [28, 32], y [20, 28]
            (34, 24, 4, 8)]      # tile 3: x [32, 36], y [20, 28]
    assert len(out) == 4
    for row, (cx, cy, w, h) in zip(out, want):
        assert row[:2] == [0.0, 1.0] and np.allclose(row[2:], [cx / S, cy / S, w / S, h / S], rtol=0, atol=1e-12), (row, cx, cy, w, h)
    only0 = P.mosaic_yolo_labels([rows, [], [], []], [(H0, W0)] * 4, [g] * 4, (32, 20), S)
    assert only0 == out[:1]
    # orientation 1 (x -> 40 - x: R x [24, 32]) in tile 1 under the corner rule for the centre (32, 40): offsets (32, 40 - 30): x [56, 64], y [16, 28]
    out = P.mosaic_yolo_labels([[], rows, [], []], [(H0, W0)] * 4, [g, [40, 30, 32, 10, 1, 0, 0, 0], g, g], (32, 40), S)
    assert len(out) == 1 and np.allclose(out[0][2:], [60 / S, 22 / S, 8 / S, 12 / S], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        P.mosaic_yolo_labels([rows] * 3, [(H0, W0)] * 3, [g] * 3, (32, 20), S)


def test_each_drop_rule_at_a_tile_edge():
    W0, H0, S = 100, 50, 64
    rows, sizes = [[1, 0.3, 0.4, 0.2, 0.4]], [(H0, W0)] * 4
    tile0 = lambda g, centre, **kw: P.mosaic_yolo_labels([rows, [], [], []], sizes, [g] * 4, centre, S, **kw)
    # canvas x [31, 39], y [16, 28]; tile 0 of centre (32, 40) leaves x [31, 32]: 1 px wide, 12 of 96 in area, ratio 12
    g = [40, 30, 23, 10, 0, 0, 0, 0]
    assert tile0(g, (32, 40)) == [] and len(tile0(g, (32, 40), min_px=0.5)) == 1
    assert len(P.augment_yolo_labels(rows, W0, H0, g, S)) == 1                      # on the whole canvas it stays
    # canvas x [28, 36], y [16, 28]; tile 0 of centre (32, 18) leaves 4 x 2 = 8 of 96 in area: 0.083
    g = [40, 30, 20, 10, 0, 0, 0, 0]
    assert tile0(g, (32, 18)) == [] and len(tile0(g, (32, 18), min_area_ratio=0.05)) == 1
    # 640 canvas, box x [160, 480], y [300, 340]; tile 0 of centre (640, 302) leaves 320 x 2: ratio 160 (area rule relaxed in both calls)
    sliver, gs = [[0, 0.5, 0.5, 0.5, 40 / 640]], [640, 640, 0, 0, 0, 0, 0, 0]
    args = ([sliver, [], [], []], [(640, 640)] * 4, [gs] * 4, (640, 302), 640)
    assert P.mosaic_yolo_labels(*args, min_area_ratio=0.01) == [] and len(P.mosaic_yolo_labels(*args, min_area_ratio=0.01, max_aspect=200.0)) == 1
    # wholly in another tile, and an empty tile: no area left
    assert tile0([40, 30, 32, 10, 0, 0, 0, 0], (32, 40), min_px=0.0) == []
    assert tile0(g, (0, 40), min_px=0.0) == [] and tile0(g, (32, 0), min_px=0.0) == []


def test_labels_at_the_degenerate_centre_are_augment_yolo_labels():
    rng = np.random.default_rng(5)
    S, sizes = 64, [(90, 60), (50, 120), (64, 64), (33, 47)]
    geom = P.sample_geometry(sizes * 50, S, rng, scale=(0.3, 2.5), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5).reshape(50, 4, 8)
    geom[:, :, 2:4] += rng.integers(-25, 26, size=(50, 4, 2)).astype(np.int32)
    kept = 0
    for g4 in geom:
        rows = [[[float(rng.integers(0, 2)), *rng.uniform(0.0, 1.0, 2), *rng.uniform(-0.05, 0.6, 2)] for _ in range(4)] for _ in range(4)]
        want = P.augment_yolo_labels(rows[0], sizes[0][1], sizes[0][0], g4[0], S)
        assert P.mosaic_yolo_labels(rows, sizes, g4, (S, S), S) == want             # exactly: the default clip is the whole canvas
        for kw in (dict(min_px=0.0), dict(min_area_ratio=0.5, max_aspect=3.0)):
            assert P.mosaic_yolo_labels(rows, sizes, g4, (S, S), S, **kw) == P.augment_yolo_labels(rows[0], sizes[0][1], sizes[0][0], g4[0], S, **kw)
        kept += len(want)
    assert 20 < kept < 200


def test_mask_and_label_move_together():
    """One filled rectangle per tile is both mask and box: after the sampled mosaic its visible bounding box inside the tile is the returned row."""
    S, sources = 64, [(90, 60), (50, 120), (64, 64), (33, 47)]
    rng = np.random.default_rng(64)
    sizes = sources * 50                                                              # 200 canvases
    index, geom, centres = P.sample_mosaic(sizes, S, rng, prob=1.0, centre=(0.25, 0.75), scale=(0.5, 1.0), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)
    kept = small = 0
    for i in range(len(sizes)):
        rects = rectangles(centres[i], S)
        for t in range(4):
            H0, W0 = sizes[index[i, t]]
            g = geom[i, t]
            x1, y1 = int(rng.integers(0, W0 - 1)), int(rng.integers(0, H0 - 1))
            x2, y2 = int(rng.integers(x1 + 1, W0 + 1)), int(rng.integers(y1 + 1, H0 + 1))
            mask = np.zeros((H0, W0), np.uint8)
            mask[y1:y2, x1:x2] = 255
            row = [[0, (x1 + x2) / 2 / W0, (y1 + y2) / 2 / H0, (x2 - x1) / W0, (y2 - y1) / H0]]
            rows4 = [row if k == t else [] for k in range(4)]
            sizes4 = [sizes[k] for k in index[i]]
            _, m = augment(np.zeros((H0, W0, 3), np.uint8), mask, g, S)
            tx0, ty0, tx1, ty1 = rects[t]
            ys, xs = np.nonzero(m[0, ty0:ty1, tx0:tx1])
            ys, xs = ys + ty0, xs + tx0
            ext_w, ext_h = (int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)) if len(xs) else (0, 0)
            out = P.mosaic_yolo_labels(rows4, sizes4, geom[i], centres[i], S)
            if out:
                kept += 1
                tol = 1 + max(g[0] / W0, g[1] / H0)
                _, _, cx, cy, w, h = out[0]
                box = [(cx - w / 2) * S, (cy - h / 2) * S, (cx + w / 2) * S, (cy + h / 2) * S]
                assert len(xs), (i, t, g)
                seen = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
                assert max(abs(a - b) for a, b in zip(box, seen)) <= tol, (i, t, g, box, seen)
                assert tx0 <= box[0] and box[2] <= tx1 and ty0 <= box[1] and box[3] <= ty1
            elif P.mosaic_yolo_labels(rows4, sizes4, geom[i], centres[i], S, min_px=0.0):   # dropped by the size rule alone
                small += 1
                assert min(ext_w, ext_h) < 2.0 + 1, (i, t, g, ext_w, ext_h)
    print(f"kept {kept} of 800, dropped by the size rule alone {small}")
    assert kept >= 200 and small >= 1


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


GOOD = [32, 16, 0, 0, 0, 0, 0, 0]


def _call(lib, n=1, S=64, geom=None, stride=8, tiles=True, centres=None, lut=None, out=PTR, out_m=PTR, edit=None, geom_null=False, centres_null=False):
    descs = (L.RawImage * (4 * max(n, 1)))()
    for d in descs:
        d.bgr, d.mask, d.height, d.width, d.row_stride, d.mask_row_stride = PTR, PTR, 10, 20, 60, 20
    if edit:
        edit(descs)
    rows = [GOOD for _ in range(4 * n)] if geom is None else geom
    flat = (C.c_int32 * (8 * 4 * max(n, 1)))(*[v for r in rows for v in r])
    cen = [(32, 17)] * n if centres is None else centres
    cflat = (C.c_int32 * (2 * max(n, 1)))(*[v for c in cen for v in c])
    return lib.mtbt_mosaic_batch(descs if tiles else None, n, S, None if geom_null else flat, stride, None if centres_null else cflat, lut, out, out_m, None)


def test_symbol_and_additive_abi(lib):
    assert "mtbt_mosaic_batch" in L.SYMBOLS and hasattr(lib, "mtbt_mosaic_batch")
    assert len(L.SYMBOLS["mtbt_mosaic_batch"][1]) == 10 and L.SYMBOLS["mtbt_mosaic_batch"][0] is C.c_int
    assert lib.mtbt_abi_version() == 5 == L.ABI_VERSION
    assert len(L.ARG_STRUCTS) == 10 and lib.mtbt_sizeof_args(9) > 0 and lib.mtbt_sizeof_args(10) == -1
    assert _call(lib, n=0) == 0                                                     # nothing to do, nothing launched


def test_bad_arguments_are_refused_before_any_launch(lib):
    assert _call(lib, tiles=False) == EINVAL
    assert _call(lib, geom_null=True) == EINVAL
    assert _call(lib, centres_null=True) == EINVAL
    assert _call(lib, out=None) == EINVAL
    assert _call(lib, n=-1) == EINVAL
    for stride in (7, 9, 0):
        assert _call(lib, stride=stride) == EINVAL
    for S in (62, 0, -64):
        assert _call(lib, S=S) == EINVAL
    for centre in ((-4, 10), (68, 10), (30, 10), (2, 2), (32, -1), (32, 65), (-1, -1)):
        assert _call(lib, centres=[centre]) == EINVAL, centre
        assert _call(lib, n=10, centres=[(32, 17)] * 8 + [centre, (32, 17)]) == EINVAL, centre     # canvas 9 of 10: the second launch chunk
    for field, values in ((0, (0, -1, 32769)), (1, (0, -5, 32769)), (4, (8, -1, 12)), (5, (1,)), (6, (-1,)), (7, (7,))):
        for v in values:
            row = list(GOOD)
            row[field] = v
            for t in range(4):
                rows = [GOOD] * 4
                rows[t] = row
                assert _call(lib, geom=rows) == EINVAL, (field, v, t)
                assert _call(lib, geom=rows, centres=[(64, 64)]) == EINVAL, (field, v, t)            # also where the tile is empty
                assert _call(lib, n=10, geom=[GOOD] * 32 + rows + [GOOD] * 4) == EINVAL, (field, v, t)   # canvas 9 of 10: still before the first launch

    def bad(at, **kw):
        def edit(descs):
            for k, v in kw.items():
                setattr(descs[len(descs) - 4 + at], k, v)
        return edit
    for kw in (dict(bgr=None), dict(height=0), dict(width=-3), dict(row_stride=59), dict(mask_row_stride=19), dict(height=1 << 20, row_stride=1 << 11)):
        for t in range(4):
            assert _call(lib, edit=bad(t, **kw)) == EINVAL, (kw, t)
            assert _call(lib, centres=[(64, 64)], edit=bad(t, **kw)) == EINVAL, (kw, t)             # a bad descriptor in an empty tile
            assert _call(lib, n=9, edit=bad(t, **kw)) == EINVAL, (kw, t)
    assert _call(lib, out=PTR + 4) == EALIGN
    assert _call(lib, out_m=PTR + 8) == EALIGN
    assert _call(lib, n=10, out=PTR + 4) == EALIGN
    for centre in ((0, 0), (64, 64), (0, 64), (64, 0), (4, 1), (60, 63)):                            # legal centres, empty rectangles included
        assert _call(lib, centres=[centre], out=PTR + 4) == EALIGN, centre
    assert _call(lib, S=62, out=PTR + 4) == EINVAL                                  # the argument checks come first
    assert _call(lib, centres=[(30, 10)], out=PTR + 4) == EINVAL
