"""Training augmentation without a GPU: the numpy restatement (tests/augment_reference.py) against the letterbox oracle, the host
side of `preprocess` (geometry and table sampling, label arithmetic, pixel / label consistency) and the argument checks of
`mtbt_augment_batch` and `mtbt_letterbox_batch`, which refuse a bad call before any launch.  The reference project has no augmentation: the arithmetic is
the project's own definition (include/mtbt_hip.h)."""
import ctypes as C

import numpy as np
import pytest

from oracle import preprocess as O
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import preprocess as P

from augment_reference import augment

EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch


def _img(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8)


# ---- the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(480, 640), (37, 91), (1, 5), (64, 63)])
def test_reference_at_identity_is_the_letterbox_oracle(size):
    S = 64
    img, mask = _img(*size, seed=size[0])
    geom = P.letterbox_geometry([size], S)
    x, m = augment(img, mask, geom[0], S)
    rx, rm, _ = O.letterbox(img, mask, S)
    assert np.array_equal(x, rx) and np.array_equal(m, rm)
    x, m = augment(img, None, geom[0], S, lut=P.photometric_lut(0.0, 1.0, 1.0)[0])      # identity table, no mask
    assert np.array_equal(x, rx) and not m.any()


def test_reference_orientation_offset_and_table():
    S = 16
    img, mask = _img(8, 12, 3)
    mask = ((mask > 127) * 255).astype(np.uint8)
    pad = np.float32(114) / np.float32(255)
    base, bm = augment(img, mask, [12, 8, 0, 0, 0, 0, 0, 0], S)                    # same size: R is the source itself
    assert np.array_equal(base[:, :8, :12], (img[:, :, ::-1].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    assert np.all(base[:, 8:] == pad) and np.all(base[:, :, 12:] == pad)
    for orient in range(8):
        x, m = augment(img, mask, [12, 8, 2, 3, orient, 0, 0, 0], S)
        qh, qw = (12, 8) if orient & 4 else (8, 12)
        for y, xx in ((0, 0), (qh - 1, 0), (1, qw - 2)):                             # the definition, pixel by pixel
            x1, y1 = (qw - 1 - xx if orient & 1 else xx), (qh - 1 - y if orient & 2 else y)
            xs, ys = (y1, x1) if orient & 4 else (x1, y1)
            assert np.array_equal(x[:, 3 + y, 2 + xx], base[:, ys, xs]) and m[0, 3 + y, 2 + xx] == bm[0, ys, xs], (orient, y, xx)
        assert np.all(x[:, :3] == pad) and np.all(x[:, :, :2] == pad) and not m[0, :3].any()
    x, m = augment(img, mask, [12, 8, -11, -7, 0, 0, 0, 0], S)                      # one pixel visible
    assert np.array_equal(x[:, 0, 0], base[:, 7, 11]) and np.all(x.reshape(3, -1)[:, 1:] == pad)
    for off in ((-12, 0), (0, -8), (16, 0), (0, 16), (-1000, 5)):                    # wholly outside: pure pad
        x, m = augment(img, mask, [12, 8, off[0], off[1], 0, 0, 0, 0], S)
        assert np.all(x == pad) and not m.any()
    lut = np.stack([np.full(256, 7, np.uint8), np.arange(256, dtype=np.uint8)[::-1], np.arange(256, dtype=np.uint8)])   # B, G, R
    x, _ = augment(img, mask, [12, 8, 0, 0, 0, 0, 0, 0], S, lut=lut)
    assert np.all(x[2, :8, :12] == np.float32(7) / np.float32(255))                  # plane 2 = B = table row 0
    assert np.array_equal(x[1, :8, :12], (255 - img[:, :, 1]).astype(np.float32) / np.float32(255))
    assert np.array_equal(x[0], base[0]) and np.all(x[:, 8:] == pad)                # the pad is not remapped


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def test_sample_geometry_is_seeded_and_stays_in_range():
    S = 64
    sizes = [(90, 60), (50, 120), (7, 300), (64, 64)] * 250
    kw = dict(scale=(0.4, 2.5), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)
    g = P.sample_geometry(sizes, S, np.random.default_rng(11), **kw)
    assert g.dtype == np.int32 and g.shape == (1000, 8)
    assert np.array_equal(g, P.sample_geometry(sizes, S, np.random.default_rng(11), **kw))
    assert not np.array_equal(g, P.sample_geometry(sizes, S, np.random.default_rng(12), **kw))
    assert not g[:, 5:].any() and set(np.unique(g[:, 4])) == set(range(8))
    for (H0, W0), (nw, nh, ox, oy, orient) in zip(sizes, g[:, :5].tolist()):
        s = S / max(H0, W0)
        lo, hi = 0.4 * np.exp(-0.3), 2.5 * np.exp(0.3)
        assert max(1, int(W0 * s * lo)) <= nw <= max(1, int(W0 * s * hi) + 1) and max(1, int(H0 * s * lo)) <= nh <= max(1, int(H0 * s * hi) + 1)
        qw, qh = (nh, nw) if orient & 4 else (nw, nh)
        for off, q in ((ox, qw), (oy, qh)):
            assert min(0, S - q) <= off <= max(0, S - q)        # inside the padding, or a crop window: never pushed out while pad shows
    assert len(np.unique(g[:, 2])) > 20
    top = P.sample_geometry(sizes, S, np.random.default_rng(11), place="topleft", **kw)
    assert not top[:, 2:4].any() and np.array_equal(top[:, [0, 1, 4]], g[:, [0, 1, 4]])
    with pytest.raises(ValueError):
        P.sample_geometry(sizes, S, np.random.default_rng(0), place="centre")


def test_sample_geometry_all_off_is_letterbox_geometry():
    sizes = [(480, 640), (1000, 700), (37, 91), (1, 5), (5, 1), (3000, 11), (64, 63), (640, 640)]
    for S in (64, 640):
        g = P.sample_geometry(sizes, S, np.random.default_rng(3), scale=(1, 1), aspect=0.0, fliplr=0.0, flipud=0.0, transpose=0.0, place="topleft")
        want = P.letterbox_geometry(sizes, S)
        assert np.array_equal(g, want)
        for (H0, W0), row in zip(sizes, want.tolist()):
            sc = S / max(H0, W0)
            assert row == [max(1, int(W0 * sc)), max(1, int(H0 * sc)), 0, 0, 0, 0, 0, 0]


def test_photometric_tables():
    ident = P.photometric_lut(0.0, 1.0, 1.0)
    assert ident.shape == (1, 3, 256) and ident.dtype == np.uint8 and np.array_equal(ident[0], np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    b, c, g = np.array([0.2, -0.2, 0.0, 0.1]), np.array([0.8, 1.2, 0.01, 3.0]), np.array([0.8, 1.25, 1.0, 0.5])
    t = P.photometric_lut(b, c, g)
    assert t.shape == (4, 3, 256) and np.all(np.diff(t.astype(np.int32), axis=2) >= 0)        # monotone for contrast > 0
    assert np.array_equal(t[:, 0], t[:, 1]) and np.array_equal(t[:, 0], t[:, 2])
    v = 100
    assert t[0, 0, v] == int(np.rint(255 * (0.8 * ((v / 255) ** 0.8 - 0.5) + 0.5 + 0.2)))
    assert t[3].min() == 0 and t[3].max() == 255                                                    # clipped
    s = P.sample_photometric(5, np.random.default_rng(2))
    assert s.shape == (5, 3, 256) and np.array_equal(s, P.sample_photometric(5, np.random.default_rng(2)))
    assert np.array_equal(P.sample_photometric(3, np.random.default_rng(2), brightness=0.0, contrast=0.0, gamma=0.0), np.repeat(ident, 3, 0))


# ---- labels --------------------------------------------------------------------------------------------------------------------
def test_labels_under_the_eight_orientations_by_hand():
    # source 100 x 50, box x [20, 40], y [10, 30];  R is 40 x 30: x [8, 16], y [6, 18];  offsets (5, -3);  S = 64
    W0, H0, S = 100, 50, 64
    rows = [[1, 0.3, 0.4, 0.2, 0.4]]
    want = {0: (17, 9, 8, 12),     # x [13, 21], y [3, 15]
            1: (33, 9, 8, 12),     # x -> 40 - x: [24, 32] + 5
            2: (17, 15, 8, 12),    # y -> 30 - y: [12, 24] - 3
            3: (33, 15, 8, 12),
            4: (17, 9, 12, 8),     # transposed, Q is 30 x 40: x [6, 18] + 5, y [8, 16] - 3
            5: (23, 9, 12, 8),     # x -> 30 - x: [12, 24] + 5
            6: (17, 25, 12, 8),    # y -> 40 - y: [24, 32] - 3
            7: (23, 25, 12, 8)}
    for orient, (cx, cy, w, h) in want.items():
        out = P.augment_yolo_labels(rows, W0, H0, [40, 30, 5, -3, orient, 0, 0, 0], S)
        assert len(out) == 1 and out[0][:2] == [0.0, 1.0]
        assert np.allclose(out[0][2:], [cx / S, cy / S, w / S, h / S], rtol=0, atol=1e-12), (orient, out)
    # clipping: offsets (-10, -3) cut x [8, 16] to [0, 6] and y [6, 18] to [3, 15]
    out = P.augment_yolo_labels(rows, W0, H0, [40, 30, -10, -3, 0, 0, 0, 0], S)
    assert np.allclose(out[0][2:], [3 / S, 9 / S, 6 / S, 12 / S], rtol=0, atol=1e-12)
    assert P.augment_yolo_labels([[1, 0.5], [0, 0.5, 0.5, 0.0, 0.2]], W0, H0, [40, 30, 0, 0, 0, 0, 0, 0], S) == []      # malformed, empty


def test_each_drop_rule():
    W0, H0, S = 100, 50, 64
    g = [40, 30, 0, 0, 0, 0, 0, 0]
    thin = [[0, 0.5, 0.5, 0.04, 0.5]]                            # 4 source pixels wide -> 1.6 px
    assert P.augment_yolo_labels(thin, W0, H0, g, S) == [] and len(P.augment_yolo_labels(thin, W0, H0, g, S, min_px=1.5)) == 1
    big = [[0, 0.5, 0.5, 0.8, 0.8]]                              # R x [4, 36]; offset -33 leaves x [0, 3]: 3 px of 32 = 0.094 of the area
    gc = [40, 30, -33, 0, 0, 0, 0, 0]
    assert P.augment_yolo_labels(big, W0, H0, gc, S) == [] and len(P.augment_yolo_labels(big, W0, H0, gc, S, min_area_ratio=0.05)) == 1
    gs = [640, 640, 0, 0, 0, 0, 0, 0]
    sliver = [[0, 0.5, 0.5, 0.5, 2.5 / 640]]                     # 320 x 2.5 px: ratio 128
    assert P.augment_yolo_labels(sliver, 640, 640, gs, 640) == [] and len(P.augment_yolo_labels(sliver, 640, 640, gs, 640, max_aspect=200.0)) == 1
    gone = P.augment_yolo_labels(big, W0, H0, [40, 30, 64, 0, 0, 0, 0, 0], S, min_px=0.0)       # wholly outside: no area left
    assert gone == []


def test_labels_at_identity_follow_transform_yolo_labels():
    rng = np.random.default_rng(5)
    rows = [[float(rng.integers(0, 2)), *rng.uniform(0.0, 1.0, 2), *rng.uniform(-0.05, 0.6, 2)] for _ in range(200)]
    W0, H0, S = 1234, 777, 640
    g = P.letterbox_geometry([(H0, W0)], S)[0]
    kept = 0
    for r in rows:
        a = P.augment_yolo_labels([r], W0, H0, g, S)
        if a:
            t = P.transform_yolo_labels([r], W0, H0, S / max(H0, W0), S)
            assert len(t) == 1 and t[0][:2] == a[0][:2]
            assert np.abs(np.array(a[0][2:]) - np.array(t[0][2:])).max() <= 1.0 / S
            kept += 1
    assert 50 < kept < 200


@pytest.mark.parametrize("size", [(90, 60), (50, 120)])
def test_mask_and_label_move_together(size):
    """The mask is a filled rectangle equal to the box: after any geometry its visible bounding box is the returned row."""
    S, (H0, W0) = 64, size
    rng = np.random.default_rng(H0)
    img = np.zeros((H0, W0, 3), np.uint8)
    sizes = [size] * 200
    geom = P.sample_geometry(sizes, S, rng, scale=(0.3, 2.5), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)
    geom[:, 2:4] += rng.integers(-25, 26, size=(200, 2)).astype(np.int32)          # also partly and wholly outside the canvas
    kept = small = 0
    for g in geom:
        x1, y1 = int(rng.integers(0, W0 - 1)), int(rng.integers(0, H0 - 1))
        x2, y2 = int(rng.integers(x1 + 1, W0 + 1)), int(rng.integers(y1 + 1, H0 + 1))
        mask = np.zeros((H0, W0), np.uint8)
        mask[y1:y2, x1:x2] = 255
        row = [[0, (x1 + x2) / 2 / W0, (y1 + y2) / 2 / H0, (x2 - x1) / W0, (y2 - y1) / H0]]
        _, m = augment(img, mask, g, S)
        ys, xs = np.nonzero(m[0])
        ext_w, ext_h = (int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)) if len(xs) else (0, 0)
        out = P.augment_yolo_labels(row, W0, H0, g, S)
        if out:
            kept += 1
            tol = 1 + max(g[0] / W0, g[1] / H0)
            _, _, cx, cy, w, h = out[0]
            box = [(cx - w / 2) * S, (cy - h / 2) * S, (cx + w / 2) * S, (cy + h / 2) * S]
            assert len(xs), g
            seen = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
            assert max(abs(a - b) for a, b in zip(box, seen)) <= tol, (g, box, seen)
        elif P.augment_yolo_labels(row, W0, H0, g, S, min_px=0.0):                  # dropped by the size rule alone
            small += 1
            assert min(ext_w, ext_h) < 2.0 + 1, (g, ext_w, ext_h)
    assert kept > 50 and small > 0


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _call(lib, n=1, S=64, geom=None, stride=8, images=True, lut=None, out=PTR, out_m=PTR, edit=None, geom_null=False):
    descs = (L.RawImage * max(n, 1))()
    for d in descs:
        d.bgr, d.mask, d.height, d.width, d.row_stride, d.mask_row_stride = PTR, PTR, 10, 20, 60, 20
    if edit:
        edit(descs)
    rows = [[32, 16, 0, 0, 0, 0, 0, 0] for _ in range(n)] if geom is None else geom
    flat = (C.c_int32 * (8 * max(n, 1)))(*[v for r in rows for v in r])
    return lib.mtbt_augment_batch(descs if images else None, n, S, None if geom_null else flat, stride, lut, out, out_m, None)


def test_symbol_and_additive_abi(lib):
    assert "mtbt_augment_batch" in L.SYMBOLS and hasattr(lib, "mtbt_augment_batch")
    assert len(L.SYMBOLS["mtbt_augment_batch"][1]) == 9 and L.SYMBOLS["mtbt_augment_batch"][0] is C.c_int
    assert lib.mtbt_abi_version() == 5 == L.ABI_VERSION
    assert len(L.ARG_STRUCTS) == 10 and lib.mtbt_sizeof_args(9) > 0 and lib.mtbt_sizeof_args(10) == -1
    assert _call(lib, n=0) == 0                                                     # nothing to do, nothing launched


def test_bad_arguments_are_refused_before_any_launch(lib):
    assert _call(lib, images=False) == EINVAL
    assert _call(lib, geom_null=True) == EINVAL
    assert _call(lib, out=None) == EINVAL
    assert _call(lib, n=-1) == EINVAL
    for stride in (7, 9, 0):
        assert _call(lib, stride=stride) == EINVAL
    for S in (62, 0, -64):
        assert _call(lib, S=S) == EINVAL
    good = [32, 16, 0, 0, 0, 0, 0, 0]
    for field, values in ((0, (0, -1, 32769)), (1, (0, -5, 32769)), (4, (8, -1, 12)), (5, (1,)), (6, (-1,)), (7, (7,))):
        for v in values:
            row = list(good)
            row[field] = v
            assert _call(lib, geom=[row]) == EINVAL, (field, v)
            assert _call(lib, n=40, geom=[good] * 39 + [row]) == EINVAL, (field, v)     # in the second launch chunk: still before the first launch

    def bad(**kw):
        def edit(descs):
            for k, v in kw.items():
                setattr(descs[len(descs) - 1], k, v)
        return edit
    for kw in (dict(bgr=None), dict(height=0), dict(width=-3), dict(row_stride=59), dict(mask_row_stride=19), dict(height=1 << 20, row_stride=1 << 11)):
        assert _call(lib, edit=bad(**kw)) == EINVAL, kw
        assert _call(lib, n=33, edit=bad(**kw)) == EINVAL, kw
    assert _call(lib, out=PTR + 4) == EALIGN
    assert _call(lib, out_m=PTR + 8) == EALIGN
    assert _call(lib, S=62, out=PTR + 4) == EINVAL                                  # the argument checks come first


def _letterbox_call(lib, n=1, S=64, images=True, out=PTR, out_m=PTR, edit=None):
    descs = (L.RawImage * max(n, 1))()
    for d in descs:
        d.bgr, d.mask, d.height, d.width, d.row_stride, d.mask_row_stride = PTR, PTR, 10, 20, 60, 20
    if edit:
        edit(descs)
    return lib.mtbt_letterbox_batch(descs if images else None, n, S, out, out_m, None, None)


def test_letterbox_bad_arguments_are_refused_before_any_launch(lib):
    """The letterbox follows the order of the two newer entry points: every descriptor first (also one in the second launch chunk, which
    used to be refused only after the first chunk had been launched), then the alignment."""
    assert _letterbox_call(lib, n=0) == 0
    assert _letterbox_call(lib, images=False) == EINVAL
    assert _letterbox_call(lib, out=None) == EINVAL
    assert _letterbox_call(lib, n=-1) == EINVAL
    for S in (62, 0, -64):
        assert _letterbox_call(lib, S=S) == EINVAL

    def bad(index, **kw):
        def edit(descs):
            for k, v in kw.items():
                setattr(descs[index], k, v)
        return edit
    for kw in (dict(bgr=None), dict(height=0), dict(width=-3), dict(row_stride=59), dict(mask_row_stride=19), dict(height=1 << 20, row_stride=1 << 11),
               dict(width=-2 ** 31)):
        assert _letterbox_call(lib, edit=bad(0, **kw)) == EINVAL, kw
        assert _letterbox_call(lib, n=40, edit=bad(39, **kw)) == EINVAL, kw             # second chunk of 32: still before the first launch
        assert _letterbox_call(lib, n=40, out=PTR + 4, edit=bad(39, **kw)) == EINVAL, kw
    assert _letterbox_call(lib, out=PTR + 4) == EALIGN
    assert _letterbox_call(lib, out_m=PTR + 8) == EALIGN
    assert _letterbox_call(lib, S=62, out=PTR + 4) == EINVAL
    assert _letterbox_call(lib, out_m=PTR + 8, edit=bad(0, width=0)) == EINVAL


def test_invalid_and_misaligned_is_invalid(lib):
    bad_row = [32, 16, 0, 0, 8, 0, 0, 0]
    assert _call(lib, geom=[bad_row], out=PTR + 4) == EINVAL
    assert _call(lib, geom=[bad_row], out_m=PTR + 8) == EINVAL
    assert _call(lib, n=40, geom=[[32, 16, 0, 0, 0, 0, 0, 0]] * 39 + [bad_row], out=PTR + 4) == EINVAL
    assert _call(lib, out=PTR + 4) == EALIGN
