"""CPU checks of the distance transform and the region terms of the segmentation loss: tests/edt_reference.py (the yardstick of the GPU
tests) is held against outside definitions -- scipy's exact Euclidean transform, Kervadec et al.'s `one_hot2dist`, torch autograd in
float64 -- and the entry points and wrappers refuse bad arguments before any launch, without a device."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage as scipy_ndimage

import edt_reference as R
from multitask_bonetumor_yolo_amd import TrainStep, _lib as L, build as B, distance_transform, seg_region_loss, signed_distance


def scipy_d2(targets: np.ndarray) -> np.ndarray:
    """Squared distance to the nearest True pixel as exact integers: scipy's nearest-target INDICES, the distance recomputed from them."""
    idx = scipy_ndimage.distance_transform_edt(~targets, return_distances=False, return_indices=True).astype(np.int64)
    yy, xx = np.mgrid[0:targets.shape[0], 0:targets.shape[1]]
    return (idx[0] - yy) ** 2 + (idx[1] - xx) ** 2


@pytest.mark.parametrize("shape", R.SHAPES)
def test_reference_maps_match_scipy(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for name, m in R.plane_cases(rng, *shape):
        d_set, d_unset = R.d2_maps(m, pairs=True)
        for what, targets, got in (("set", m, d_set), ("unset", ~m, d_unset)):
            if targets.any():
                assert np.array_equal(got, scipy_d2(targets)), (name, what)
                assert got.max() < 2 ** 29 and np.array_equal(got == 0, targets), (name, what)
            else:                                # scipy leaves a plane without a target undefined; the contract says the sentinel
                assert (got == R.NONE).all(), (name, what)
            assert np.array_equal(R.d2_separable(targets), got), (name, what)   # the search the 640 x 640 GPU case uses


def test_reference_phi_is_kervadecs_one_hot2dist():
    rng = np.random.default_rng(5)
    edt = scipy_ndimage.distance_transform_edt
    for name, pos in R.plane_cases(rng, 37, 64):
        phi = R.phi_of(pos, *R.d2_maps(pos))
        if pos.all():                            # their formula takes edt of a plane without background: the contract defines 0
            assert (phi == 0).all()
            continue
        res = np.zeros(pos.shape)
        if pos.any():                            # boundary-loss utils.py, one_hot2dist
            neg = ~pos
            res = edt(neg) * neg - (edt(pos) - 1) * pos
        assert np.array_equal(phi, res), name
        assert (phi[pos] <= 0).all() and (phi[~pos] >= 0).all()


@pytest.mark.parametrize("w_dice,w_boundary,smooth", [(1.0, 0.0, 1.0), (0.0, 1.0, 1.0), (0.7, 0.01, 0.5)])
def test_reference_terms_and_gradients_match_autograd(w_dice, w_boundary, smooth):
    rng = np.random.default_rng(11)
    H, W = 19, 23
    masks = np.stack([R.blobs(rng, H, W, 1), np.zeros((H, W), bool), np.ones((H, W), bool), rng.uniform(size=(H, W)) < 0.3])
    phi = np.stack([R.phi_of(m, *R.d2_maps(m)) for m in masks])
    z = rng.uniform(-6, 6, size=masks.shape)
    dice, boundary, total, grad = R.region_terms(z, masks, phi, w_dice=w_dice, w_boundary=w_boundary, smooth=smooth)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    t, ph = torch.tensor(masks, dtype=torch.float64), torch.tensor(phi, dtype=torch.float64)
    p = torch.sigmoid(zt)
    inter, denom = (p * t).sum((1, 2)), p.sum((1, 2)) + t.sum((1, 2))      # MONAI DiceLoss(sigmoid=True), per sample, smooth_nr = smooth_dr
    t_dice = (1.0 - (2.0 * inter + smooth) / (denom + smooth)).mean()
    t_boundary = (ph * p).mean()                                           # Kervadec's SurfaceLoss: mean of probs * dist_maps
    t_total = w_dice * t_dice + w_boundary * t_boundary
    t_total.backward()
    t_dice, t_boundary, t_total = t_dice.detach(), t_boundary.detach(), t_total.detach()
    assert dice == pytest.approx(float(t_dice), rel=1e-12) and boundary == pytest.approx(float(t_boundary), rel=1e-12, abs=1e-15)
    assert total == pytest.approx(float(t_total), rel=1e-12)
    np.testing.assert_allclose(grad, zt.grad.numpy(), rtol=1e-10, atol=1e-18)
    assert phi[1].max() == phi[1].min() == 0 and phi[2].max() == phi[2].min() == 0   # the empty and the full plane contribute nothing


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


P = 4096          # a non-NULL, 16-byte aligned dummy: no refused call dereferences it


def edt_args(**kw):
    a = L.DistanceTransformArgs()
    a.packed, a.workspace, a.d2_set, a.d2_unset = P, P, P, P
    a.n, a.H, a.W, a.pitch = 2, 37, 130, 24
    a.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_distance_transform_refuses_before_any_launch(lib):
    q = lib.mtbt_distance_transform_workspace_bytes
    assert q(0, 37, 130) == 0 and q(2, 37, 130) >= 2 * 2 * 37 * 192 * 2 and q(70, 37, 130) == q(64, 37, 130)
    assert q(-1, 37, 130) == q(1, 0, 130) == q(1, 37, 0) == q(1, 16385, 1) == q(1, 1, 16385) == -1 and q(1, 16384, 16384) > 0
    call = lambda a: lib.mtbt_distance_transform(C.byref(a), None)
    assert lib.mtbt_distance_transform(None, None) == -1
    for bad in (dict(packed=None), dict(d2_set=None, d2_unset=None), dict(workspace=None), dict(n=-1), dict(H=0), dict(W=0), dict(H=16385),
                dict(W=16385, pitch=8 * 257), dict(pitch=16), dict(pitch=32), dict(workspace_bytes=q(2, 37, 130) - 1)):
        assert call(edt_args(**bad)) == -1, bad
    for bad in (dict(packed=P + 4), dict(workspace=P + 8), dict(d2_set=P + 2), dict(d2_unset=P + 1)):
        assert call(edt_args(**bad)) == -2, bad
    assert call(edt_args(n=0)) == 0 and call(edt_args(n=0, workspace=None, workspace_bytes=0)) == 0      # launches nothing
    assert lib.mtbt_sizeof_distance_args(0) == C.sizeof(L.DistanceTransformArgs) and lib.mtbt_sizeof_distance_args(2) == -1


def region_args(**kw):
    a = L.SegRegionArgs()
    a.logits, a.targets, a.d2_set, a.d2_unset, a.d_logits, a.workspace, a.out = P, P, P, P, P, P, P
    a.B, a.H, a.W, a.pitch = 3, 37, 130, 24
    a.workspace_bytes = 1 << 40
    a.smooth, a.w_dice, a.w_boundary = 1.0, 1.0, 0.01
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_seg_region_loss_refuses_before_any_launch(lib):
    q = lib.mtbt_seg_region_loss_workspace_bytes
    assert q(3, 37, 130) > 0 and q(0, 37, 130) == q(65536, 37, 130) == q(3, 0, 130) == q(3, 37, 16385) == -1
    call = lambda a: lib.mtbt_seg_region_loss(C.byref(a), None)
    assert lib.mtbt_seg_region_loss(None, None) == -1
    for bad in (dict(logits=None), dict(targets=None), dict(out=None), dict(workspace=None), dict(B=0), dict(H=0), dict(W=16385, pitch=8 * 257),
                dict(pitch=16), dict(smooth=-1.0), dict(w_dice=-0.5), dict(w_boundary=float("nan")), dict(w_dice=float("inf")),
                dict(d2_set=None), dict(d2_unset=None), dict(d2_set=None, d2_unset=None), dict(accumulate=2),
                dict(workspace_bytes=q(3, 37, 130) - 1)):
        assert call(region_args(**bad)) == -1, bad
    for bad in (dict(targets=P + 4), dict(workspace=P + 8), dict(logits=P + 2), dict(bias=P + 1), dict(d2_set=P + 2), dict(d_logits=P + 3), dict(out=P + 2)):
        assert call(region_args(**bad)) == -2, bad
    assert lib.mtbt_sizeof_distance_args(1) == C.sizeof(L.SegRegionArgs)


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    packed = torch.zeros(2, 37, 24, dtype=torch.uint8)
    with pytest.raises(ValueError, match="to = "):
        distance_transform(packed, 130, to="nearest")
    for fn in (lambda: distance_transform(packed, 130), lambda: distance_transform(packed, 130, to="both"), lambda: signed_distance(packed, 130)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    z, m = torch.zeros(3, 1, 37, 130), torch.zeros(3, 1, 37, 130)
    with pytest.raises(RuntimeError, match="no CPU path"):
        seg_region_loss(z, m)
    with pytest.raises(ValueError, match="seg_logits"):
        seg_region_loss(z.double(), m)
    with pytest.raises(ValueError, match="seg_logits"):
        seg_region_loss(torch.zeros(3, 2, 37, 130), m)
    with pytest.raises(ValueError, match="does not fit"):
        seg_region_loss(z, torch.zeros(3, 1, 37, 128))
    with pytest.raises(ValueError, match="packed gt_masks"):
        seg_region_loss(z, torch.zeros(3, 37, 16, dtype=torch.uint8), W=130)
    with pytest.raises(ValueError, match="packed gt_masks"):
        seg_region_loss(z, torch.zeros(3, 37, 24, dtype=torch.uint8), W=129)
    for kw in (dict(dice_weight=-1.0), dict(boundary_weight=-0.1), dict(smooth=float("nan"))):
        with pytest.raises(ValueError, match=">= 0"):
            seg_region_loss(z, m, **kw)


@pytest.mark.parametrize("kw", [dict(seg_dice_weight=-1.0), dict(seg_boundary_weight=-0.01), dict(seg_dice_smooth=-1.0), dict(seg_dice_weight=float("nan"))])
def test_trainstep_refuses_negative_region_weights(kw):
    with pytest.raises(ValueError, match="seg_dice_weight, seg_boundary_weight"):
        TrainStep(None, (2, 3, 64, 64), **kw)                  # refused before the model is looked at
