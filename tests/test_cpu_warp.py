"""CPU checks of the affine warp (include/mtbt_hip.h `mtbt_warp_batch`): tests/warp_reference.py against its stated exact properties and
against an independent float64 bilinear sample, the host logic (coefficients, their exact inverse, the draws, the label moves), labels
against pixels, and the entry point's refusals (none of which launches anything)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import polygon_reference as PR
import warp_reference as R
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import preprocess as P

S16, H0, W0 = 16, 11, 13
IDENTITY = [65536, 0, 0, 0, 65536, 0, 0, 0]


def source(seed=0, h=H0, w=W0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def forward(angle, scale, shear, S, h, w, shift=(0.0, 0.0), flip=False):
    """Source edge coordinates -> canvas edge coordinates: centre on centre (+ shift), R(angle) . [[1, shear], [0, 1]] . scale."""
    t = math.radians(angle)
    lin = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]) @ np.array([[1.0, shear], [0.0, 1.0]]) * scale
    if flip:
        lin = lin @ np.diag([-1.0, 1.0])
    F = np.zeros((2, 3))
    F[:, :2] = lin
    F[:, 2] = np.array([S / 2 + shift[0], S / 2 + shift[1]]) - lin @ np.array([w / 2, h / 2])
    return F


MAPS = [(33.0, 1.3, 0.1), (-170.0, 0.4, -0.2), (7.0, 3.0, 0.0)]


# ---- 1. the reference against itself: the three exact properties -------------------------------------------------------------------
def test_identity_reproduces_the_source():
    src = source(1)
    v, inside = R.warp_bytes(src, IDENTITY, S16)
    assert int(inside.sum()) == H0 * W0 and inside[:H0, :W0].all()
    assert np.array_equal(v[:H0, :W0], src) and not v[~inside].any()
    assert np.array_equal(P.affine_coefficients(np.array([[1.0, 0, 0], [0, 1.0, 0]]))[0], IDENTITY)   # the identity in edge coordinates too
    img_t, mask_t = R.warp(src, None, IDENTITY, S16)
    assert img_t.dtype == np.float32 and img_t.shape == (3, S16, S16) and not mask_t.any()
    assert np.array_equal(img_t[:, :H0, :W0], (src[:, :, ::-1].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    assert (img_t[:, ~inside] == np.float32(114) / np.float32(255)).all()


def test_quarter_turn_is_a_transpose_of_the_flipped_source():
    src = source(2)
    v, inside = R.warp_bytes(src, [0, 65536, 0, -65536, 0, (H0 - 1) << 16, 0, 0], S16)
    want = np.transpose(src[::-1], (1, 0, 2))                                  # [W0, H0, 3]
    assert int(inside.sum()) == H0 * W0 and inside[:W0, :H0].all()
    assert np.array_equal(v[:W0, :H0], want)


def test_half_pixel_shift_is_the_rounded_mean():
    src = source(3)
    v, inside = R.warp_bytes(src, [65536, 0, 32768, 0, 65536, 0, 0, 0], S16)
    s = src.astype(int)
    right = s[:, np.minimum(np.arange(W0) + 1, W0 - 1)]
    # position x + 0.5 lies inside up to x = W0 - 2 (W0 - 1 + 0.5 is the footprint's open end)
    assert inside[:H0, :W0 - 1].all() and not inside[:, W0 - 1:].any()
    assert np.array_equal(v[:H0, :W0 - 1], ((s + right + 1) >> 1)[:, :W0 - 1].astype(np.uint8))


# ---- 2. the reference against a float64 bilinear sample at the exact rational position ---------------------------------------------
def float_sample(src, coef_row, S):
    """(value float64 [S, S, C], lo, hi of the four taps) at X / 65536, Y / 65536 exactly (float64 holds |X| < 2^48 and the quotient)."""
    a, b, c, d, e, f = (int(v) for v in coef_row[:6])
    dy, dx = np.mgrid[0:S, 0:S]
    px, py = (a * dx + b * dy + c) / 65536.0, (d * dx + e * dy + f) / 65536.0
    h, w = src.shape[:2]
    sx, sy = np.floor(px), np.floor(py)
    fx, fy = (px - sx)[..., None], (py - sy)[..., None]
    cl = lambda v, n: np.clip(v, 0, n - 1).astype(int)
    s = src.astype(np.float64)
    t00, t01, t10, t11 = s[cl(sy, h), cl(sx, w)], s[cl(sy, h), cl(sx + 1, w)], s[cl(sy + 1, h), cl(sx, w)], s[cl(sy + 1, h), cl(sx + 1, w)]
    val = (1 - fx) * (1 - fy) * t00 + fx * (1 - fy) * t01 + (1 - fx) * fy * t10 + fx * fy * t11
    return val, px, py


def rule_taps(src, coef_row, S):
    """min and max of the four taps the RULE blends, per pixel and channel."""
    h, w = src.shape[:2]
    Xs, Ys, _ = R.positions(coef_row, S, h, w)
    sx, sy = Xs >> 5, Ys >> 5
    x0, x1, y0, y1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1), np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    taps = np.stack([src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]]).astype(np.float64)
    return taps.min(axis=0), taps.max(axis=0)


@pytest.mark.parametrize("k,want_inside", [(0, 212), (1, 23), (2, 256)])
def test_reference_within_the_derived_bound_of_a_float64_sample(k, want_inside):
    """The position is rounded by at most 1/64 px per axis and the bilinear surface is continuous across cells, so the blend moves by at
    most (2 / 64) (max - min of the four taps); the final >> 10 rounds by at most 0.5."""
    angle, scale, shear = MAPS[k]
    src = source(10 + k)
    coef = P.affine_coefficients(forward(angle, scale, shear, S16, H0, W0))[0]
    v, inside = R.warp_bytes(src, coef, S16)
    val, px, py = float_sample(src, coef, S16)
    lo, hi = rule_taps(src, coef, S16)
    err = np.abs(v.astype(np.float64) - val)[inside]
    bound = (0.5 + (2.0 / 64.0) * (hi - lo))[inside]
    n = int(inside.sum())
    print(f"map {MAPS[k]}: {n} of {S16 * S16} inside, worst error / bound {float((err / bound).max()):.3f}")
    assert 0 < n <= S16 * S16 and n == want_inside
    assert (err <= bound).all()
    # a second opinion on interior pixels: scipy's order-1 interpolation is the same float64 sample
    interior = inside & (px >= 0) & (px <= W0 - 1) & (py >= 0) & (py <= H0 - 1)
    assert interior.sum() > n // 2
    for c in range(3):
        sp = ndimage.map_coordinates(src[:, :, c].astype(np.float64), [py[interior], px[interior]], order=1)
        assert np.abs(sp - val[..., c][interior]).max() < 1e-9


def test_a_map_wholly_outside_is_pure_pad():
    src, mask = source(4), np.full((H0, W0), 255, dtype=np.uint8)
    lut = np.random.default_rng(5).integers(0, 256, (3, 256), dtype=np.uint8)
    for shift in ((100.0, 0.0), (0.0, -100.0), (-40.0, 60.0)):
        coef = P.affine_coefficients(forward(33.0, 1.3, 0.1, S16, H0, W0, shift=shift))[0]
        v, inside = R.warp_bytes(src, coef, S16)
        assert not inside.any()
        img_t, mask_t = R.warp(src, mask, coef, S16, lut=lut)                   # the table must not touch the pad
        assert (img_t == np.float32(114) / np.float32(255)).all() and not mask_t.any()


def test_nearest_mask_rule():
    mask = np.random.default_rng(6).integers(0, 256, (H0, W0), dtype=np.uint8)
    m, inside = R.warp_nearest(mask, IDENTITY, S16)
    assert np.array_equal(m[:H0, :W0], mask) and int(inside.sum()) == H0 * W0
    _, mask_t = R.warp(source(6), mask, IDENTITY, S16)
    assert np.array_equal(mask_t[0, :H0, :W0], (mask >= 128).astype(np.float32))
    # a shift of 0.5 - 1/32 px still reads the pixel itself, 0.5 px reads the next one
    m, _ = R.warp_nearest(mask, [65536, 0, 32768 - 2048, 0, 65536, 0, 0, 0], S16)
    assert np.array_equal(m[:H0, :W0 - 1], mask[:, :W0 - 1])
    m, _ = R.warp_nearest(mask, [65536, 0, 32768, 0, 65536, 0, 0, 0], S16)
    assert np.array_equal(m[:H0, :W0 - 1], mask[:, 1:])


# ---- 3. host logic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,h,w", [(64, 37, 53), (640, 768, 1024), (1024, 3000, 2000)])
def test_forward_of_the_integer_map_differs_from_the_matrix_by_the_rounding_only(S, h, w):
    """G = F^-1 has each of its six numbers rounded by at most 2^-17, so for a canvas point p with 0 <= p <= S the source position moves by
    at most delta = 2^-17 (2 S + 1) per axis; with q = G(p): F(q) = p and F~(q) = p - L~ delta, L~ the linear part of F~ (that of F up to
    the same rounding): |F~(q) - F(q)| <= ||L||_inf 2^-17 (2 S + 1), taken with 1 % of slack for L~ against L and float64 evaluation."""
    rng = np.random.default_rng(S)
    for _ in range(50):
        F = P.sample_affine([(h, w)], S, rng, scale=(0.4, 2.5), aspect=0.3, degrees=180.0, shear=20.0, translate=0.3, fliplr=0.5, flipud=0.5)[0]
        Fq = P.affine_forward(P.affine_coefficients(F))[0]
        assert Fq.dtype == np.float64 and Fq.shape == (2, 3)
        Linv = np.linalg.inv(F[:, :2])
        bound = np.abs(F[:, :2]).sum(axis=1).max() * 2.0 ** -17 * (2 * S + 1) * 1.01
        assert bound < 0.1                                                      # a few 2^-16 S pixels: far below anything a label rule sees
        for p in ((0, 0), (S, 0), (0, S), (S, S)):
            q = Linv @ (np.array(p, dtype=np.float64) - F[:, 2])
            assert np.abs(F[:, :2] @ q + F[:, 2] - p).max() < 1e-9
            assert np.abs(Fq[:, :2] @ q + Fq[:, 2] - p).max() <= bound
    # exactly representable maps come back exactly
    for F in (np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[0.0, -2.0, 40.0], [2.0, 0.0, -8.0]]), np.array([[-0.5, 0, 16.0], [0, 0.25, 3.0]])):
        assert np.array_equal(P.affine_forward(P.affine_coefficients(F))[0], F)


def test_sample_affine_is_reproducible_and_draws_in_the_documented_order():
    sizes, S = [(300, 200), (128, 256), (77, 91)], 160
    kw = dict(scale=(0.7, 1.4), aspect=0.2, degrees=30.0, shear=8.0, translate=0.15, fliplr=0.5, flipud=0.5)
    F = P.sample_affine(sizes, S, np.random.default_rng(5), **kw)
    assert F.shape == (3, 2, 3) and F.dtype == np.float64
    assert np.array_equal(F, P.sample_affine(sizes, S, np.random.default_rng(5), **kw))
    r0, r1 = np.random.default_rng(5), np.random.default_rng(5)
    P.sample_affine(sizes, S, r0, **kw)
    g, a = r1.uniform(0.7, 1.4, 3), np.exp(r1.uniform(-0.2, 0.2, 3))
    th, sx, sy = (np.deg2rad(r1.uniform(-v, v, 3)) for v in (30.0, 8.0, 8.0))
    tx, ty = r1.uniform(-0.15, 0.15, 3), r1.uniform(-0.15, 0.15, 3)
    lr, ud = r1.random(3) < 0.5, r1.random(3) < 0.5
    assert r0.bit_generator.state == r1.bit_generator.state
    for i, (h, w) in enumerate(sizes):
        s = S / max(h, w)
        kx, ky = s * g[i] * a[i] * (-1 if lr[i] else 1), s * g[i] / a[i] * (-1 if ud[i] else 1)
        rot = np.array([[math.cos(th[i]), -math.sin(th[i])], [math.sin(th[i]), math.cos(th[i])]])
        lin = rot @ np.array([[1, math.tan(sx[i])], [math.tan(sy[i]), 1]]) @ np.diag([kx, ky])
        assert np.allclose(F[i, :, :2], lin, rtol=1e-12, atol=1e-12)
        # the image's centre lands on the canvas centre plus the translation
        assert np.allclose(F[i, :, :2] @ [w / 2, h / 2] + F[i, :, 2], [S / 2 + tx[i] * S, S / 2 + ty[i] * S], rtol=1e-12, atol=1e-9)
    # the defaults without rotation, shear, shift and flips are the centred letterbox scale
    F = P.sample_affine([(100, 50)], 64, np.random.default_rng(0), scale=(1.0, 1.0), degrees=0.0, translate=0.0, fliplr=0.0)[0]
    assert np.allclose(F, [[0.64, 0, 16.0], [0, 0.64, 0.0]], atol=1e-12)


def test_singular_and_out_of_limit_matrices_raise():
    for bad in ([[1.0, 2.0, 0], [2.0, 4.0, 0]], [[0.0, 0, 0], [0, 0, 0]], [[np.nan, 0, 0], [0, 1.0, 0]], [[np.inf, 0, 0], [0, 1.0, 0]]):
        with pytest.raises(ValueError, match="singular"):
            P.affine_coefficients(np.array(bad))
    with pytest.raises(ValueError, match="limits"):
        P.affine_coefficients(np.array([[1.0 / 1025, 0, 0], [0, 1.0, 0]]))      # 1025 source px per canvas px
    with pytest.raises(ValueError, match="limits"):
        P.affine_coefficients(np.array([[1.0, 0, -2.0 ** 31 - 2], [0, 1.0, 0]]))  # an offset beyond 2^47 / 65536 px
    assert P.affine_coefficients(np.array([[1.0 / 1024, 0, 0], [0, -1.0 / 1024, 0]]))[0, [0, 4]].tolist() == [1 << 26, -(1 << 26)]
    with pytest.raises(ValueError):
        P.affine_coefficients(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="singular"):
        P.affine_forward(np.array([[1, 2, 0, 2, 4, 0, 0, 0]]))
    with pytest.raises(ValueError):
        P.affine_forward(np.zeros((1, 8)))                                       # floats are not coefficient rows


def _turn(angle, S, h, w):
    return P.affine_forward(P.affine_coefficients(forward(angle, 1.0, 0.0, S, h, w)))[0]


def test_box_under_a_quarter_turn_is_the_transposed_box():
    S, h, w = 128, 80, 100
    (row,) = P.affine_yolo_labels([[3, 0.5, 0.5, 0.4, 0.2]], w, h, _turn(90.0, S, h, w), S)
    assert row[:2] == [0.0, 3.0]
    assert np.allclose(row[2:], [0.5, 0.5, 0.2 * h / S, 0.4 * w / S], atol=1e-6)   # 40 x 16 px -> 16 x 40 px about the centre
    (row,) = P.affine_yolo_labels([[3, 0.3, 0.6, 0.2, 0.3]], w, h, _turn(90.0, S, h, w), S)
    # (x, y) about the centre -> (-y, x): the box centre (30, 48) - (50, 40) = (-20, 8) -> (-8, -20) + (64, 64)
    assert np.allclose(row[2:], [56 / S, 44 / S, 0.3 * h / S, 0.2 * w / S], atol=1e-6)


def test_box_under_45_degrees_has_sides_w_plus_h_over_root_2():
    S, h, w = 256, 100, 100
    bw, bh = 0.4 * w, 0.2 * h
    (row,) = P.affine_yolo_labels([[1, 0.5, 0.5, 0.4, 0.2]], w, h, _turn(45.0, S, h, w), S)
    side = (bw + bh) / math.sqrt(2.0)
    assert np.allclose(row[2:], [0.5, 0.5, side / S, side / S], atol=1e-4)      # the integer map's rounding: ~0.006 px of 256
    # the polygon of the same rectangle has the same hull; a polygon that is not a rectangle stays tight (a diamond turns into a square)
    (prow, v), = P.affine_polygons([[1, 0.3, 0.4, 0.7, 0.4, 0.7, 0.6, 0.3, 0.6]], w, h, _turn(45.0, S, h, w), S)
    assert np.allclose(prow, row, atol=1e-9) and v.shape == (4, 2)
    (drow, _), = P.affine_polygons([[1, 0.5, 0.3, 0.7, 0.5, 0.5, 0.7, 0.3, 0.5]], w, h, _turn(45.0, S, h, w), S)
    assert np.allclose(drow[4:], [20 * math.sqrt(2.0) / S] * 2, atol=1e-4)         # the box of the diamond was 40 x 40: it shrank


def test_affine_polygons_on_a_rectangle_equals_affine_yolo_labels_on_the_box():
    rng = np.random.default_rng(13)
    S, kept, dropped = 64, 0, 0
    for it in range(600):
        w, h = int(rng.integers(20, 200)), int(rng.integers(20, 200))
        Fq = P.affine_forward(P.affine_coefficients(P.sample_affine([(h, w)], S, rng, scale=(0.5, 2.5), aspect=0.3, degrees=180.0, shear=10.0,
                                                                    translate=0.4, flipud=0.5)))[0]
        xc, yc, bw, bh = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.02, 0.6), rng.uniform(0.02, 0.6)
        rect = None if it % 3 else tuple(int(v) for v in (rng.integers(0, 32), rng.integers(0, 32), rng.integers(32, 65), rng.integers(32, 65)))
        x1, y1, x2, y2 = xc - bw / 2, yc - bh / 2, xc + bw / 2, yc + bh / 2
        box = P.affine_yolo_labels([[1, xc, yc, bw, bh]], w, h, Fq, S, clip_rect=rect)
        pol = P.affine_polygons([[1, x1, y1, x2, y1, x2, y2, x1, y2]], w, h, Fq, S, clip_rect=rect)
        assert len(box) == len(pol)
        dropped += not box
        if box:
            kept += 1
            assert box[0] == pol[0][0]
            v = pol[0][1]
            assert v.dtype == np.float64 and np.allclose(v[0], Fq[:, :2] @ [x1 * w, y1 * h] + Fq[:, 2], atol=1e-9)   # vertices are not clipped
            r = rect or (0, 0, S, S)
            assert r[0] / S - 1e-12 <= box[0][2] - box[0][4] / 2 and box[0][2] + box[0][4] / 2 <= r[2] / S + 1e-12
    assert kept > 150 and dropped > 50
    assert P.affine_yolo_labels([[1, 0.5, 0.5, 0.0, 0.2], [1, 0.5, 0.5]], 64, 64, _turn(10.0, 64, 64, 64), 64) == []


def test_augment_polygons_results_are_where_they_were():
    """Two cases of the polygon tests restated with their pinned values: the tail now shared with `affine_polygons` moved nothing."""
    g = [64, 64, 0, 0, 0, 0, 0, 0]
    (row6, v), = P.augment_polygons([[2, -0.5, 0.25, 0.5, 0.25, 0.5, 0.75, -0.5, 0.75]], 64, 64, g, 64)
    assert row6 == [0.0, 2.0, 0.25, 0.5, 0.5, 0.5] and v[:, 0].min() == -32.0
    tri = [0, 0.1, 0.1, 0.5, 0.1, 0.3, 0.6]
    assert len(P.augment_polygons([tri], 64, 64, g, 64)) == 1
    assert P.augment_polygons([[0, 0.1, 0.1, 0.3, 0.3, 0.5, 0.5]], 64, 64, g, 64) == []
    assert P.augment_polygons([[0, 0.1, 0.1, 0.12, 0.1, 0.11, 0.6]], 64, 64, g, 64) == []
    assert P.augment_polygons([tri], 64, 64, g, 64, clip_rect=(0, 0, 8, 8)) == []
    bar = [[0, 0.0, 0.25, 1.0, 0.25, 1.0, 0.2578125, 0.0, 0.2578125]]
    assert P.augment_polygons(bar, 640, 640, [640, 640, 0, 0, 0, 0, 0, 0], 640) == []
    assert len(P.augment_polygons(bar, 640, 640, [640, 640, 0, 0, 0, 0, 0, 0], 640, max_aspect=200.0)) == 1
    # a flipped, transposed, shifted triangle, computed by hand: x' = y 2, y' = x 0.5, then x' -> 128 - x', plus (3, -4)
    (row6, v), = P.augment_polygons([tri], 64, 64, [32, 128, 3, -4, 5, 0, 0, 0], 256)
    assert np.allclose(v, [[128 - 12.8 + 3, 3.2 - 4], [128 - 12.8 + 3, 16 - 4], [128 - 76.8 + 3, 9.6 - 4]], atol=1e-12)
    assert np.allclose(row6, [0.0, 0.0, (54.2 + 118.2) / 2 / 256, 6.0 / 256, 64.0 / 256, 12.0 / 256], atol=1e-12)


# ---- 4. labels follow pixels -------------------------------------------------------------------------------------------------------
def _chebyshev_to_edges(px, py, poly):
    """Smallest Chebyshev distance from the points (px, py) to the segments of the closed polygon: max(|u1 + t v1|, |u2 + t v2|) is convex
    and piecewise linear in t, so its minimum over [0, 1] is at an end, at a zero of a term or where the two terms are equal in size."""
    best = np.full(px.shape, np.inf)
    for i in range(len(poly)):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % len(poly)]
        u1, u2, v1, v2 = ax - px, ay - py, bx - ax, by - ay
        cands = [np.zeros_like(px), np.ones_like(px)]
        with np.errstate(divide="ignore", invalid="ignore"):
            for num, den in ((-u1, v1), (-u2, v2), (u2 - u1, v1 - v2), (-u1 - u2, v1 + v2)):
                cands.append(np.clip(np.nan_to_num(num / den, nan=0.0, posinf=0.0, neginf=0.0), 0.0, 1.0) if den != 0 else np.zeros_like(px))
        for t in cands:
            best = np.minimum(best, np.maximum(np.abs(u1 + t * v1), np.abs(u2 + t * v2)))
    return best


@pytest.mark.parametrize("scale,bound", [(1.0, 1.0), (2.0, 2.0)])
def test_labels_follow_pixels(scale, bound):
    """The nearest tap moves a sample by at most 0.5 + 1/64 source px per axis, which is at most scale (0.5 + 1/64) (|cos| + |sin|) <= 0.73
    scale canvas px in Chebyshev terms at 30 degrees; the two fills quantise their vertices to 1/16 px.  So a canvas pixel can differ only
    within `bound` = 1 px (scale 1) or 2 px (scale 2) of an edge of the moved polygon."""
    h, w, S = 48, 60, 128
    seg_row = [0, 0.25, 0.2, 0.7, 0.3, 0.8, 0.75, 0.5, 0.55, 0.3, 0.8]
    poly_src = np.asarray(seg_row[1:]).reshape(-1, 2) * [w, h]
    src_mask = PR.fill([poly_src], h, w).astype(np.uint8) * 255
    coef = P.affine_coefficients(forward(30.0, scale, 0.0, S, h, w))
    warped = R.warp_nearest(src_mask, coef[0], S)[0] >= 128
    (row6, verts), = P.affine_polygons([seg_row], w, h, P.affine_forward(coef)[0], S)
    assert verts.min() > 2 and verts.max() < S - 2                               # the whole polygon is on the canvas
    moved = PR.fill([verts], S, S)
    diff = warped != moved
    assert warped.sum() > 200 * scale * scale and moved.sum() > 200 * scale * scale
    ys, xs = np.nonzero(diff)
    dist = _chebyshev_to_edges(xs + 0.5, ys + 0.5, verts)
    print(f"scale {scale}: {int(diff.sum())} of {int(moved.sum())} pixels differ, farthest {float(dist.max()) if len(dist) else 0.0:.3f} px from an edge")
    assert (dist <= bound).all()
    # the label box is the moved polygon's, tight
    assert np.allclose([row6[2] * S, row6[3] * S, row6[4] * S, row6[5] * S],
                       [(verts[:, 0].min() + verts[:, 0].max()) / 2, (verts[:, 1].min() + verts[:, 1].max()) / 2, np.ptp(verts[:, 0]), np.ptp(verts[:, 1])])


# ---- 5. the boundary ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def desc(**kw):
    d = dict(bgr=1 << 20, mask=1 << 22, height=64, width=48, row_stride=144, mask_row_stride=48)
    d.update(kw)
    im = L.RawImage()
    for k, v in d.items():
        setattr(im, k, v)
    return im


def call(lib, items, rows=None, S=64, out=1 << 30, out_m=1 << 31, stride=8, count=None, images=True, coef=True):
    n = len(items) if count is None else count
    arr = (L.RawImage * max(len(items), 1))(*items)
    k = np.ascontiguousarray(np.tile(np.array(IDENTITY, dtype=np.int64), (max(len(items), 1), 1)) if rows is None else np.asarray(rows, dtype=np.int64))
    return lib.mtbt_warp_batch(arr if images else None, n, S, k.ctypes.data_as(C.POINTER(C.c_int64)) if coef else None, stride, None, out, out_m, None)


def test_symbol_and_chunk_are_exported(lib):
    assert hasattr(lib, "mtbt_warp_batch") and "mtbt_warp_batch" in L.SYMBOLS
    assert L.WARP_CHUNK in (16, 24, 32) and L.ABI_VERSION == 5
    assert (L.WARP_LIN_MAX, L.WARP_OFF_MAX) == (R.LIN_MAX, R.OFF_MAX) == (1 << 26, 1 << 47)


def test_entry_point_refuses_in_the_documented_order_before_any_launch(lib):
    """No GPU here: a call that got as far as a launch would not return MTBT_EINVAL / MTBT_EALIGN.  A valid call with a misaligned output
    is MTBT_EALIGN, which shows that the arguments before it were accepted."""
    EINVAL, EALIGN = -1, -2
    assert call(lib, [desc()], out=24) == EALIGN and call(lib, [desc()], out_m=24) == EALIGN and call(lib, [desc()], out=24, out_m=None) == EALIGN
    assert call(lib, [desc()], images=False) == EINVAL and call(lib, [desc()], coef=False) == EINVAL and call(lib, [desc()], out=None) == EINVAL
    for stride in (0, 6, 7, 9, 16):
        assert call(lib, [desc()], stride=stride) == EINVAL
    assert call(lib, [desc()], count=-1) == EINVAL
    for S in (0, -4, 2, 63, 32772, 1 << 20):
        assert call(lib, [desc()], S=S) == EINVAL
    assert call(lib, [desc()], S=32768, out=24) == EALIGN                       # the largest canvas is accepted
    # coefficients: the limits themselves pass, one beyond does not; reserved fields must be zero
    for j, lim in ((0, 1 << 26), (1, 1 << 26), (3, 1 << 26), (4, 1 << 26), (2, 1 << 47), (5, 1 << 47)):
        for sign in (1, -1):
            row = list(IDENTITY)
            row[j] = sign * lim
            assert call(lib, [desc()], [row], out=24) == EALIGN, (j, sign)
            row[j] = sign * (lim + 1)
            assert call(lib, [desc()], [row]) == EINVAL, (j, sign)
            assert call(lib, [desc(), desc(), desc()], [IDENTITY, IDENTITY, row]) == EINVAL   # the last row is checked before any launch
        row = list(IDENTITY)
        row[j] = -(1 << 63)
        assert call(lib, [desc()], [row]) == EINVAL
    for j in (6, 7):
        row = list(IDENTITY)
        row[j] = 1
        assert call(lib, [desc()], [row]) == EINVAL
    # descriptors: what mtbt_letterbox_batch refuses
    for bad in (dict(bgr=None), dict(height=0), dict(width=0), dict(height=-3), dict(row_stride=143), dict(mask_row_stride=47),
                dict(height=(1 << 31) // 144 + 1)):
        assert call(lib, [desc(**bad)]) == EINVAL, bad
        assert call(lib, [desc(), desc(), desc(**bad)]) == EINVAL, bad
        assert lib.mtbt_letterbox_batch((L.RawImage * 1)(desc(**bad)), 1, 64, 1 << 30, 1 << 31, None, None) == EINVAL, bad
    assert call(lib, [desc(mask=None, mask_row_stride=0)], out=24) == EALIGN   # no mask is fine
    # invalid and misaligned together is MTBT_EINVAL
    assert call(lib, [desc(height=0)], out=24) == EINVAL
    assert call(lib, [desc()], [[1 << 27, 0, 0, 0, 65536, 0, 0, 0]], out=24, out_m=24) == EINVAL
    assert call(lib, [desc()], S=62, out=24) == EINVAL
    # an empty batch is fine and launches nothing
    assert call(lib, [desc()], count=0) == 0
    assert call(lib, [desc()], count=0, out=24) == EALIGN


def test_python_refusals_need_no_device(lib):
    g = torch.zeros(32, 32, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        P.warp_batch([], None, np.zeros((0, 8), dtype=np.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.warp_batch([g], None, np.array([IDENTITY]))


# ---- draws of the sample functions (device work stubbed) ---------------------------------------------------------------------------
SIZES = [(300, 200), (128, 256), (77, 91)]
BOX_ROWS = [[[0, 0.5, 0.5, 0.4, 0.3]], [], [[1, 0.3, 0.6, 0.2, 0.2], [2, 0.7, 0.4, 0.5, 0.5]]]
SEG_ROWS = [[[0, 0.2, 0.2, 0.8, 0.2, 0.8, 0.8, 0.2, 0.8]], [], [[1, 0.1, 0.1, 0.6, 0.2, 0.4, 0.9]]]


@pytest.mark.parametrize("name", ["affine_samples", "affine_samples_seg"])
def test_samples_draw_affine_then_photometric_then_clahe(monkeypatch, name):
    seen = {"clahe": [], "warp": []}

    def fake_clahe(images, clip_limit=2.0, grid=(8, 8), out=None):
        seen["clahe"].append((list(clip_limit), tuple(grid)))
        return list(images)

    def fake_warp(images, masks, coef, lut=None, img_size=640):
        seen["warp"].append((np.array(coef), lut.clone()))
        return torch.zeros(len(images), 3, img_size, img_size), torch.zeros(len(images), 1, img_size, img_size)

    monkeypatch.setattr(P, "clahe_batch", fake_clahe)
    monkeypatch.setattr(P, "warp_batch", fake_warp)
    monkeypatch.setattr(P, "_upload", lambda t, dev: t)
    monkeypatch.setattr(P, "_seg_outputs", lambda per_canvas, rects, S, dev: (None, [[it[0] for it in c] for c in per_canvas], None))
    images = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES]
    kw = dict(degrees=25.0, shear=5.0, scale=(0.8, 1.2), brightness=0.1, min_px=1.0)
    run = (lambda rng, **extra: P.affine_samples_seg(images, SEG_ROWS, 160, rng, **kw, **extra)) if name.endswith("_seg") else \
          (lambda rng, **extra: P.affine_samples(images, None, BOX_ROWS, 160, rng, **kw, **extra))
    r0, r1 = np.random.default_rng(31), np.random.default_rng(31)
    plain = run(r0)
    F = P.sample_affine(SIZES, 160, r1, degrees=25.0, shear=5.0, scale=(0.8, 1.2))
    lut = P.sample_photometric(3, r1, brightness=0.1)
    assert r0.bit_generator.state == r1.bit_generator.state and seen["clahe"] == []
    coef = P.affine_coefficients(F)
    assert np.array_equal(seen["warp"][0][0], coef) and np.array_equal(seen["warp"][0][1].numpy(), lut)
    # the labels follow the integer map, not F
    Fq = P.affine_forward(coef)
    if name.endswith("_seg"):
        want = [[r6 for r6, _ in P.affine_polygons(r, w, h, Fq[i], 160, min_px=1.0)] for i, (r, (h, w)) in enumerate(zip(SEG_ROWS, SIZES))]
        assert plain[2] == want and sum(len(c) for c in want) >= 1
    else:
        want = P.collate_boxes([P.affine_yolo_labels(r, w, h, Fq[i], 160, min_px=1.0) for i, (r, (h, w)) in enumerate(zip(BOX_ROWS, SIZES))])
        assert torch.equal(plain[2], want) and want.shape[0] >= 1
    # with clahe: the same coefficients and table, then exactly the draws of sample_clahe
    r2 = np.random.default_rng(31)
    run(r2, clahe=dict(prob=0.6, grid=(4, 2)))
    expect = P.sample_clahe(3, r1, prob=0.6)
    assert r2.bit_generator.state == r1.bit_generator.state and seen["clahe"] == [(expect, (4, 2))]
    assert np.array_equal(seen["warp"][1][0], coef) and torch.equal(seen["warp"][1][1], seen["warp"][0][1])
    with pytest.raises(TypeError):
        run(np.random.default_rng(0), transpose=0.5)
