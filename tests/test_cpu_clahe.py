"""CPU checks of the CLAHE rule (include/mtbt_hip.h `mtbt_clahe_batch`): tests/clahe_reference.py against a scalar form with cv2's
redistribution loop written out in exact rationals, against a float64 form in cv2's terms, the stated properties, the host formula, the
entry point's refusals (none of which launches anything), the struct layout, and the draws of the `*_samples` functions."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import clahe_reference as R
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import preprocess as pre

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def image(rng, H, W, channels=1):
    """Half smooth, half noise, with a flat dark corner: every tile has a different histogram and some are heavily clipped."""
    y, x = np.mgrid[0:H, 0:W]
    v = 60 + 120 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.integers(-40, 41, (H, W))
    v[: H // 3, : W // 3] = 7
    g = np.clip(v, 0, 255).astype(np.uint8)
    if channels == 1:
        return g
    return np.ascontiguousarray(np.stack([g, np.clip(g.astype(int) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8),
                                          rng.integers(0, 256, (H, W)).astype(np.uint8)], axis=-1))


# ---- the scalar form: plain loops, cv2's redistribution loop, exact rationals ------------------------------------------------------
def cv2_redistribute(hist, clip):
    """clahe.cpp's clip step, loop for loop."""
    hist = [int(v) for v in hist]
    if clip <= 0:
        return hist
    clipped = 0
    for b in range(256):
        if hist[b] > clip:
            clipped += hist[b] - clip
            hist[b] = clip
    batch = clipped // 256
    residual = clipped - batch * 256
    for b in range(256):
        hist[b] += batch
    if residual != 0:
        step = max(256 // residual, 1)
        b = 0
        while b < 256 and residual > 0:
            hist[b] += 1
            b += step
            residual -= 1
    return hist


def half_up(q: Fraction) -> int:
    return (q + Fraction(1, 2)).__floor__()


def scalar_clahe(img, grid, clip):
    gx, gy = grid
    H, W = img.shape[:2]
    tw, th = -(-W // gx), -(-H // gy)
    area = tw * th
    refl = lambda i, n: i if i < n else 2 * (n - 1) - i
    key = lambda p: int(p) if img.ndim == 2 else (int(p[0]) + 2 * int(p[1]) + int(p[2]) + 2) >> 2
    luts = {}
    for j in range(gy):
        for i in range(gx):
            hist = [0] * 256
            for y in range(j * th, (j + 1) * th):
                for x in range(i * tw, (i + 1) * tw):
                    hist[key(img[refl(y, H), refl(x, W)])] += 1
            assert sum(hist) == area
            hist = cv2_redistribute(hist, clip)
            assert sum(hist) == area
            cdf, lut = 0, []
            for b in range(256):
                cdf += hist[b]
                lut.append(half_up(Fraction(255 * cdf, area)))
            luts[j, i] = lut
    out = np.zeros_like(img)
    for y in range(H):
        tyf = Fraction(2 * y + 1, 2 * th) - Fraction(1, 2)
        ty1 = tyf.__floor__()
        ya = tyf - ty1
        ty1c, ty2c = min(max(ty1, 0), gy - 1), min(max(ty1 + 1, 0), gy - 1)
        for x in range(W):
            txf = Fraction(2 * x + 1, 2 * tw) - Fraction(1, 2)
            tx1 = txf.__floor__()
            xa = txf - tx1
            tx1c, tx2c = min(max(tx1, 0), gx - 1), min(max(tx1 + 1, 0), gx - 1)
            for c in range(1 if img.ndim == 2 else 3):
                v = int(img[y, x]) if img.ndim == 2 else int(img[y, x, c])
                res = ((luts[ty1c, tx1c][v] * (1 - xa) + luts[ty1c, tx2c][v] * xa) * (1 - ya)
                       + (luts[ty2c, tx1c][v] * (1 - xa) + luts[ty2c, tx2c][v] * xa) * ya)
                if img.ndim == 2:
                    out[y, x] = half_up(res)
                else:
                    out[y, x, c] = half_up(res)
    return out


@pytest.mark.parametrize("H,W,ch,grid,clip", [(37, 53, 1, (4, 3), 6), (37, 53, 3, (4, 3), 3), (16, 16, 1, (16, 16), 0), (16, 16, 3, (16, 16), 1),
                                              (33, 70, 3, (8, 8), 2), (5, 300, 1, (16, 1), 4), (20, 17, 1, (16, 7), 1), (40, 40, 1, (1, 1), 9)])
def test_reference_equals_scalar_form(H, W, ch, grid, clip):
    img = image(np.random.default_rng(H * W + ch), H, W, ch)
    assert np.array_equal(R.clahe(img, grid, clip), scalar_clahe(img, grid, clip))


# ---- the float64 form in cv2's terms -----------------------------------------------------------------------------------------------
def float_clahe(img, grid, clip):
    """(real-valued result before rounding, rounded result): tile curves as the rule builds them, the blend in float64 with
    txf = (x + 0.5) / tw - 0.5 and so on."""
    gx, gy = grid
    H, W = img.shape[:2]
    tw, th = R.tile_size(H, W, grid)
    hist = R.clip_hists(R.tile_hists(img, grid), clip)
    lut = np.floor(np.cumsum(hist, axis=-1) * 255.0 / (tw * th) + 0.5)
    txf, tyf = (np.arange(W) + 0.5) / tw - 0.5, (np.arange(H) + 0.5) / th - 0.5
    tx1, ty1 = np.floor(txf).astype(int), np.floor(tyf).astype(int)
    xa, ya = txf - tx1, tyf - ty1
    cx = lambda t: np.clip(t, 0, gx - 1)
    cy = lambda t: np.clip(t, 0, gy - 1)
    ex = (lambda a: a[..., None]) if img.ndim == 3 else (lambda a: a)
    g = lambda ty, tx: lut[ex(cy(ty)[:, None]), ex(cx(tx)[None, :]), img.astype(int)]
    XA, YA = ex(xa[None, :] + 0 * ya[:, None]), ex(ya[:, None] + 0 * xa[None, :])
    res = (g(ty1, tx1) * (1 - XA) + g(ty1, tx1 + 1) * XA) * (1 - YA) + (g(ty1 + 1, tx1) * (1 - XA) + g(ty1 + 1, tx1 + 1) * XA) * YA
    return res, np.floor(res + 0.5).astype(np.uint8)


@pytest.mark.parametrize("H,W,ch,grid,limit", [(75, 106, 3, (4, 3), 2.0), (33, 70, 1, (8, 8), 3.0), (640, 512, 1, (2, 2), 2.0),
                                               (300, 401, 3, (8, 8), 4.0), (257, 129, 1, (5, 7), 0.0)])
def test_reference_equals_float64_form(H, W, ch, grid, limit):
    """Values whose real result lies within 1e-9 of a half are exempt (float64 may fall on either side of an exact tie), at most 1 % of
    them.  An exact tie needs an even tile side: with tw and th odd every weight 2 t - a, a is even, so the numerator is a multiple of 4
    and cannot be 2 tw th (odd multiples of 2) modulo 4 tw th.  Tiles of 27 x 25 and 9 x 5 are therefore tie-free, 256 x 320, 51 x 38 and
    26 x 37 are not; tiny even tiles (14 x 13 of the 37 x 53 case) tie too often for this form and are checked exactly, in rationals, by
    test_reference_equals_scalar_form instead."""
    img = image(np.random.default_rng(H + W), H, W, ch)
    clip = pre.clahe_clip(limit, H, W, grid)
    res, rounded = float_clahe(img, grid, clip)
    got = R.clahe(img, grid, clip)
    frac = res + 0.5 - np.floor(res + 0.5)
    tie = np.minimum(frac, 1 - frac) < 1e-9            # the real value within 1e-9 of a half: float64 may fall on either side
    print(f"{H} x {W} x {ch} grid {grid}: {int(tie.sum())} of {tie.size} values exempted, {int((got != rounded).sum())} differ at all")
    assert tie.mean() <= 0.01
    assert np.array_equal(got[~tie], rounded[~tie])
    assert np.abs(got.astype(int) - rounded.astype(int)).max() <= 1


# ---- stated properties -------------------------------------------------------------------------------------------------------------
def test_one_tile_without_clipping_is_global_equalisation():
    img = image(np.random.default_rng(1), 40, 40)
    cdf = np.cumsum(np.bincount(img.ravel(), minlength=256))
    lut = (510 * cdf + img.size) // (2 * img.size)
    assert np.array_equal(R.clahe(img, (1, 1), 0), lut[img].astype(np.uint8))


def test_constant_image():
    for v in (0, 7, 200, 255):
        img = np.full((40, 50), v, dtype=np.uint8)
        assert (R.clahe(img, (5, 4), 0) == 255).all()
    # clip 1 on 10 x 10 tiles: the bin keeps 1 of its 100, 99 are dealt out one each to bins 0, 2, 4, ...: cdf[7] = 4 + 1, 255 * 5 / 100 = 12.75
    img = np.full((40, 50), 7, dtype=np.uint8)
    assert R.tile_size(40, 50, (5, 4)) == (10, 10)
    assert (R.clahe(img, (5, 4), 1) == 13).all()


def test_three_equal_channels_equal_the_one_channel_result():
    g = image(np.random.default_rng(2), 45, 61)
    out = R.clahe(np.ascontiguousarray(np.stack([g, g, g], axis=-1)), (4, 3), 5)
    assert np.array_equal(out[..., 0], R.clahe(g, (4, 3), 5))
    assert np.array_equal(out[..., 1], out[..., 0]) and np.array_equal(out[..., 2], out[..., 0])


@pytest.mark.parametrize("clip", [0, 1, 4, 50])
def test_curves_end_at_255_and_are_monotone(clip):
    luts = R.tile_luts(image(np.random.default_rng(3), 64, 96, 3), (4, 4), clip)
    assert (luts[..., 255] == 255).all()
    assert (np.diff(luts, axis=-1) >= 0).all() and luts.min() >= 0


def test_clip_at_or_above_the_area_is_no_clipping():
    img = image(np.random.default_rng(4), 48, 48)
    area = 12 * 16
    assert R.tile_size(48, 48, (4, 3)) == (12, 16)
    for clip in (area, area + 1, 10 * area):
        assert np.array_equal(R.clahe(img, (4, 3), clip), R.clahe(img, (4, 3), 0))
    assert not np.array_equal(R.clahe(img, (4, 3), 2), R.clahe(img, (4, 3), 0))


@pytest.mark.parametrize("r", [0, 1, 100, 255])
def test_remainders_from_constructed_histograms(r):
    clip = 10
    hist = np.zeros(256, dtype=np.int64)
    hist[5::7] = 3                                     # below the clip: untouched by it
    hist[40] = clip + 2 * 256 + r - 1                  # excess 2 * 256 + r over two bins
    hist[41] = clip + 1
    excess = int(np.maximum(hist - clip, 0).sum())
    assert excess % 256 == r and excess // 256 == 2
    got = R.clip_hists(hist, clip)
    assert got.tolist() == cv2_redistribute(hist, clip)
    assert got.sum() == hist.sum()
    assert (got - np.minimum(hist, clip) - 2).sum() == r


def test_closed_form_equals_the_loop_on_random_histograms():
    rng = np.random.default_rng(5)
    for _ in range(300):
        hist = rng.integers(0, int(rng.integers(2, 400)), 256) * (rng.random(256) < rng.random())
        clip = int(rng.integers(1, 200))
        assert R.clip_hists(hist, clip).tolist() == cv2_redistribute(hist, clip)
    batch = rng.integers(0, 300, (3, 4, 256))
    assert np.array_equal(R.clip_hists(batch, 17)[2, 1], cv2_redistribute(batch[2, 1], 17))


def test_clahe_clip():
    assert pre.clahe_clip(0.0, 100, 100) == 0 and pre.clahe_clip(-1.0, 100, 100) == 0
    assert pre.clahe_clip(2.0, 1536, 2048, (8, 8)) == int(2.0 * 192 * 256 / 256) == 384
    assert pre.clahe_clip(2.0, 37, 53, (4, 3)) == max(1, int(2.0 * 14 * 13 / 256)) == 1
    assert pre.clahe_clip(0.01, 16, 16, (16, 16)) == 1        # never below 1 once clipping is on
    assert pre.clahe_clip(40.0, 33, 70, (8, 8)) == int(40.0 * 9 * 5 / 256) == 7
    assert pre.clahe_clip(3.7, 3000, 3000, (8, 8)) == int(3.7 * 375 * 375 / 256)
    for bad in ((0, 8), (8, 17)):
        with pytest.raises(ValueError):
            pre.clahe_clip(2.0, 100, 100, bad)


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def item(**kw):
    d = dict(src=1 << 20, dst=1 << 21, height=64, width=48, channels=3, clip=2, src_row_stride=144, dst_row_stride=144)
    d.update(kw)
    im = L.ClaheImage()
    for k, v in d.items():
        setattr(im, k, v)
    return im


def call(lib, items, gx=8, gy=8, ws=1 << 22, ws_bytes=None, count=None):
    n = len(items) if count is None else count
    arr = (L.ClaheImage * max(len(items), 1))(*items)
    need = lib.mtbt_clahe_workspace_bytes(arr, max(n, 0), gx, gy) if 1 <= gx <= 16 and 1 <= gy <= 16 else 1 << 20
    return lib.mtbt_clahe_batch(arr, n, gx, gy, ws, need if ws_bytes is None else ws_bytes, None)


def test_entry_point_refuses_before_any_launch(lib):
    """No GPU here: a call that got as far as a launch or a clear of the workspace would not return MTBT_EINVAL / MTBT_EALIGN."""
    assert lib.mtbt_clahe_batch(None, 1, 8, 8, 1 << 22, 1 << 20, None) == -1
    assert call(lib, [item()], count=-1) == -1
    for gx, gy in ((0, 8), (8, 0), (17, 8), (8, 17), (-1, 8)):
        assert call(lib, [item()], gx=gx, gy=gy) == -1
    for bad in (dict(src=None), dict(dst=None), dict(channels=0), dict(channels=2), dict(channels=4), dict(height=7), dict(width=7),
                dict(clip=-1), dict(src_row_stride=143), dict(dst_row_stride=143),
                dict(height=1 << 20, src_row_stride=2048, dst_row_stride=144), dict(height=1 << 20, src_row_stride=144, dst_row_stride=2048)):
        assert call(lib, [item(**bad)]) == -1, bad
        assert call(lib, [item(), item(src=1 << 24, dst=1 << 25), item(**bad)]) == -1, bad   # the last item is checked before any launch
    # height * stride at 2^31 - 1 or beyond
    assert call(lib, [item(height=(1 << 31) // 144 + 1, src=1 << 40, dst=1 << 42)]) == -1
    # area: a tile of 2^22 pixels passes the check (and stops at the workspace), one pixel more does not
    big = dict(channels=1, height=2048, width=2048, src_row_stride=2048, dst_row_stride=2048, src=1 << 40, dst=1 << 42)
    assert call(lib, [item(**big)], gx=1, gy=1, ws=24) == -2
    assert call(lib, [item(**dict(big, width=2049, src_row_stride=2049, dst_row_stride=2049))], gx=1, gy=1, ws=24) == -1
    # workspace: NULL or one byte short
    assert call(lib, [item()], ws=None) == -1
    need = lib.mtbt_clahe_workspace_bytes((L.ClaheImage * 1)(item()), 1, 8, 8)
    assert need == 64 * (1024 + 256)
    assert call(lib, [item()], ws_bytes=need - 1) == -1
    # dst may be src exactly, and must not meet a source of the call otherwise (its own shifted, other strides, another item's)
    assert call(lib, [item(dst=1 << 20)], ws=24) == -2                                   # in place is valid: only the alignment is wrong
    assert call(lib, [item(dst=(1 << 20) + 144)]) == -1
    assert call(lib, [item(dst=(1 << 20) + 64 * 144 - 1)]) == -1
    assert call(lib, [item(dst=(1 << 20) + 63 * 144 + 144)], ws=24) == -2                # the first byte after the source
    assert call(lib, [item(dst=1 << 20, dst_row_stride=160)]) == -1
    assert call(lib, [item(), item(src=1 << 24, dst=1 << 20)]) == -1
    assert call(lib, [item(dst=1 << 20), item(dst=1 << 20)]) == -1                       # the same image twice, in place
    # MTBT_EINVAL wins over MTBT_EALIGN; a misaligned workspace alone is MTBT_EALIGN; an empty batch is fine and needs no workspace
    assert call(lib, [item(clip=-1)], ws=24) == -1
    assert call(lib, [item()], ws=24) == -2
    assert call(lib, [item()], count=0, ws=None, ws_bytes=0) == 0
    assert lib.mtbt_clahe_workspace_bytes(None, 0, 8, 8) == 0
    assert lib.mtbt_clahe_workspace_bytes(None, 1, 8, 8) == -1 and lib.mtbt_clahe_workspace_bytes(None, 0, 0, 8) == -1
    assert lib.mtbt_clahe_workspace_bytes((L.ClaheImage * 1)(item()), -1, 8, 8) == -1
    assert lib.mtbt_clahe_workspace_bytes((L.ClaheImage * 3)(), 3, 16, 16) == 3 * 256 * 1280


def test_struct_layout_matches_header(lib, tmp_path):
    fields = [f for f, _ in L.ClaheImage._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){', 'printf("size %zu\\n", sizeof(mtbt_clahe_image));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbt_clahe_image, {f}));' for f in fields] + ['return 0;}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.ClaheImage) == lib.mtbt_sizeof_clahe_args(0) == 48
    for f in fields:
        assert int(out[f]) == getattr(L.ClaheImage, f).offset, f
    assert lib.mtbt_sizeof_clahe_args(1) == -1 and lib.mtbt_sizeof_clahe_args(-1) == -1


def test_python_refusals_need_no_device(lib):
    g = torch.zeros(32, 32, dtype=torch.uint8)
    assert pre.clahe_batch([g, g], [None, None]) == [g, g] and pre.clahe_batch([g], [None])[0] is g    # never reaches the library
    with pytest.raises(ValueError):
        pre.clahe_batch([])
    with pytest.raises(ValueError):
        pre.clahe_batch([g], [1.0, 2.0])
    with pytest.raises(ValueError):
        pre.clahe_batch([g], 2.0, grid=(17, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pre.clahe_batch([g], 2.0)


# ---- draws -------------------------------------------------------------------------------------------------------------------------
def test_sample_clahe():
    a = pre.sample_clahe(200, np.random.default_rng(7), prob=0.3, clip=(1.5, 2.5))
    assert a == pre.sample_clahe(200, np.random.default_rng(7), prob=0.3, clip=(1.5, 2.5))
    on = [v for v in a if v is not None]
    assert 30 <= len(on) <= 90 and all(isinstance(v, float) and 1.5 <= v < 2.5 for v in on)
    assert all(v is None for v in pre.sample_clahe(50, np.random.default_rng(0), prob=0.0))
    assert all(v is not None for v in pre.sample_clahe(50, np.random.default_rng(0), prob=1.0))
    # two vectors of B draws whatever prob is: the generator ends in the same state
    r0, r1, r2 = (np.random.default_rng(9) for _ in range(3))
    pre.sample_clahe(13, r0, prob=0.0)
    pre.sample_clahe(13, r1, prob=1.0, clip=(2.0, 3.0))
    r2.random(13), r2.uniform(0, 1, 13)
    assert r0.bit_generator.state == r1.bit_generator.state == r2.bit_generator.state
    # the values are exactly those two vectors
    r3, r4 = np.random.default_rng(11), np.random.default_rng(11)
    on, c = r4.random(6) < 0.5, r4.uniform(1.0, 4.0, 6)
    assert pre.sample_clahe(6, r3) == [float(c[i]) if on[i] else None for i in range(6)]


@pytest.fixture
def stubbed(monkeypatch):
    """The `*_samples` functions with their device work replaced by recorders: what they draw and what they hand on is host logic."""
    seen = {"clahe": [], "geom": []}

    def fake_clahe(images, clip_limit=2.0, grid=(8, 8), out=None):
        seen["clahe"].append((len(images), list(clip_limit), tuple(grid)))
        return [im if c is None else im + 1 for im, c in zip(images, clip_limit)]

    def fake_augment(images, masks, geom, lut=None, img_size=640):
        seen["geom"].append((np.array(geom), lut.clone(), [int(im.flatten()[0]) for im in images]))
        return torch.zeros(len(images), 3, img_size, img_size), torch.zeros(len(images), 1, img_size, img_size)

    def fake_mosaic(images, masks, index, geom, centres, lut=None, img_size=640):
        seen["geom"].append((np.array(geom), lut.clone(), [int(im.flatten()[0]) for im in images], np.array(index), np.array(centres)))
        return torch.zeros(len(index), 3, img_size, img_size), torch.zeros(len(index), 1, img_size, img_size)

    monkeypatch.setattr(pre, "clahe_batch", fake_clahe)
    monkeypatch.setattr(pre, "augment_batch", fake_augment)
    monkeypatch.setattr(pre, "mosaic_batch", fake_mosaic)
    monkeypatch.setattr(pre, "_upload", lambda t, dev: t)
    monkeypatch.setattr(pre, "_seg_outputs", lambda per_canvas, rects, S, dev: (None, [[it[0] for it in c] for c in per_canvas], None))
    return seen


SIZES = [(300, 200), (128, 256), (77, 91), (640, 480), (50, 60)]
BOX_ROWS = [[[0, 0.5, 0.5, 0.4, 0.3]], [], [[1, 0.3, 0.6, 0.2, 0.2], [2, 0.7, 0.4, 0.5, 0.5]], [[0, 0.5, 0.5, 0.9, 0.9]], []]
SEG_ROWS = [[[0, 0.2, 0.2, 0.8, 0.2, 0.8, 0.8, 0.2, 0.8]], [], [[1, 0.1, 0.1, 0.6, 0.2, 0.4, 0.9]], [[2, 0.3, 0.3, 0.7, 0.3, 0.5, 0.8]], []]


def _run_samples(name, rng, **kw):
    images = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES]
    fn = getattr(pre, name)
    if name.endswith("_seg"):
        return fn(images, SEG_ROWS, 160, rng, **kw)
    return fn(images, None, BOX_ROWS, 160, rng, **kw)


@pytest.mark.parametrize("name", ["augment_samples", "mosaic_samples", "augment_samples_seg", "mosaic_samples_seg"])
def test_samples_draw_clahe_last_and_nothing_without_it(stubbed, name):
    mosaic = name.startswith("mosaic")
    # without clahe: the generator is consumed as before this option existed -- the geometry draw, then the photometric draw, nothing else
    r0, r1 = np.random.default_rng(21), np.random.default_rng(21)
    plain = _run_samples(name, r0)
    if mosaic:
        pre.sample_mosaic(SIZES, 160, r1)
    else:
        pre.sample_geometry(SIZES, 160, r1)
    pre.sample_photometric(len(SIZES), r1)
    assert r0.bit_generator.state == r1.bit_generator.state
    assert stubbed["clahe"] == [] and stubbed["geom"][0][2] == [0] * len(SIZES)
    # with it: the same geometry, table and labels, then exactly the draws of sample_clahe; every image goes through clahe_batch once
    r2 = np.random.default_rng(21)
    with_clahe = _run_samples(name, r2, clahe=dict(prob=0.6, clip=(1.0, 3.0), grid=(4, 2)))
    expect = pre.sample_clahe(len(SIZES), r1, prob=0.6, clip=(1.0, 3.0))
    assert r2.bit_generator.state == r1.bit_generator.state
    assert stubbed["clahe"] == [(len(SIZES), expect, (4, 2))]
    a, b = stubbed["geom"]
    assert all(np.array_equal(x, y) for x, y in zip(a[3:], b[3:])) and np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert b[2] == [0 if c is None else 1 for c in expect]          # the equalised tensors are what the resample reads
    rows_a, rows_b = plain[-2 if name.endswith("_seg") else -1], with_clahe[-2 if name.endswith("_seg") else -1]
    assert (rows_a == rows_b) if isinstance(rows_a, list) else torch.equal(rows_a, rows_b)
    # defaults of the option, and an unknown key
    _run_samples(name, np.random.default_rng(3), clahe={})
    assert stubbed["clahe"][-1][2] == (8, 8)
    with pytest.raises(TypeError):
        _run_samples(name, np.random.default_rng(3), clahe=dict(strength=1))
