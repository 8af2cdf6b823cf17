"""`seg_region_loss` / `SegRegionLoss` (mtbt_seg_region_loss, csrc/distance_transform.hip) against the float64 restatement in
tests/edt_reference.py (held against MONAI's / Kervadec's formulas and torch autograd in tests/test_cpu_edt.py).

Tolerances: values rtol 1e-5, the fp32-parity bound of the loss path; gradients rtol 1e-4 (the gradient tolerance of
tests/test_gpu_loss.py) plus atol 1e-6 * max |reference gradient|."""
import functools

import numpy as np
import pytest
import torch

import edt_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
SHAPES = ((64, 64), (37, 130))
W_DICE, W_BOUNDARY, SMOOTH, BIAS = 0.7, 0.05, 1.0, 0.3

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import SegRegionLoss, seg_region_loss
    from multitask_bonetumor_yolo_amd.postprocess import pack_masks


@functools.lru_cache(maxsize=None)
def case(shape):
    """(logits float32 [B, H, W], masks bool [B, H, W]: one blob, one empty, one full plane, phi float64) of one shape, computed once."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    masks = np.stack([R.blobs(rng, H, W, 1), np.zeros((H, W), bool), np.ones((H, W), bool)])
    phi = np.stack([R.phi_of(m, *R.d2_maps(m)) for m in masks])
    return rng.uniform(-6, 6, size=(B, H, W)).astype(np.float32), masks, phi


def ref_of(shape, w_dice, w_boundary, bias=0.0, smooth=SMOOTH):
    z, masks, phi = case(shape)
    return R.region_terms(z.astype(np.float64) + np.float64(np.float32(bias)), masks, phi, w_dice=np.float32(w_dice).astype(np.float64),
                          w_boundary=np.float32(w_boundary).astype(np.float64), smooth=smooth)


def dev_inputs(shape):
    z, masks, _ = case(shape)
    return torch.from_numpy(z).to(DEV)[:, None], torch.from_numpy(masks).to(DEV)[:, None].float()


def check_values(res, ref):
    got = [float(v) for v in res]
    print("values", got, "reference", ref[:3])
    for g, r in zip(got, ref[:3]):
        assert g == pytest.approx(r, rel=1e-5, abs=0 if r != 0 else 1e-12)


def check_grad(got: torch.Tensor, ref: np.ndarray):
    got = got.detach().cpu().numpy().reshape(ref.shape).astype(np.float64)
    scale = np.abs(ref).max()
    print("max |grad error| / max |grad|", np.abs(got - ref).max() / max(scale, 1e-300))
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6 * scale)


@pytest.mark.parametrize("shape", SHAPES)
def test_values_and_gradients(shape):
    z, m = dev_inputs(shape)
    res, g = seg_region_loss(z, m, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=SMOOTH, with_grads=True)
    ref = ref_of(shape, W_DICE, W_BOUNDARY)
    check_values(res, ref)
    assert tuple(g["seg_logits"].shape) == (B, 1) + shape
    check_grad(g["seg_logits"], ref[3])
    # bool, uint8 and already packed targets are the same planes; [B, H, W] logits the same logits
    for name, zz, mm, kw in (("bool", z, m.bool(), {}), ("uint8", z, (m * 255).to(torch.uint8), {}),
                             ("packed", z, pack_masks(m[:, 0]), dict(W=shape[1])), ("[B, H, W]", z[:, 0], m[:, 0], {})):
        r2, g2 = seg_region_loss(zz, mm, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, with_grads=True, **kw)
        assert torch.equal(torch.stack(r2), torch.stack(res)) and torch.equal(g2["seg_logits"], g["seg_logits"]), name
    # and a second run gives the same bits
    r3, g3 = seg_region_loss(z, m, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=SMOOTH, with_grads=True)
    assert torch.equal(torch.stack(r3), torch.stack(res)) and torch.equal(g3["seg_logits"], g["seg_logits"])


@pytest.mark.parametrize("shape", SHAPES)
def test_each_weight_zero_in_turn(shape, monkeypatch):
    z, m = dev_inputs(shape)
    res, g = seg_region_loss(z, m, dice_weight=0.0, boundary_weight=W_BOUNDARY, with_grads=True)
    ref = ref_of(shape, 0.0, W_BOUNDARY)
    check_values(res, ref)
    check_grad(g["seg_logits"], ref[3])
    # with boundary_weight = 0 the maps are never requested, and the boundary element is 0
    from multitask_bonetumor_yolo_amd import loss as loss_mod

    def never(*a, **k):
        raise AssertionError("distance_transform called with boundary_weight = 0")

    monkeypatch.setattr(loss_mod, "distance_transform", never)
    res, g = seg_region_loss(z, m, dice_weight=W_DICE, boundary_weight=0.0, with_grads=True)
    ref = ref_of(shape, W_DICE, 0.0)
    assert float(res[1]) == 0.0
    check_values((res[0], res[2]), (ref[0], ref[2]))
    check_grad(g["seg_logits"], ref[3])


@pytest.mark.parametrize("shape", SHAPES)
def test_bias_accumulate_and_smooth(shape):
    z, m = dev_inputs(shape)
    bias = torch.tensor([BIAS], device=DEV)
    res, g = seg_region_loss(z, m, bias=bias, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=0.25, with_grads=True)
    ref = ref_of(shape, W_DICE, W_BOUNDARY, bias=BIAS, smooth=0.25)
    check_values(res, ref)
    check_grad(g["seg_logits"], ref[3])
    assert not torch.equal(res[0], seg_region_loss(z, m, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=0.25)[0])   # the bias counts
    # accumulate=True: prefilled + gradient, one fp32 addition per element
    pre = torch.randn(B, *shape, device=DEV)
    buf = pre.clone()
    r2 = seg_region_loss(z, m, bias=bias, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=0.25, grad_out=buf, accumulate=True)
    assert torch.equal(torch.stack(r2[0]), torch.stack(res)) and r2[1]["seg_logits"].data_ptr() == buf.data_ptr()
    assert torch.equal(buf, pre + g["seg_logits"][:, 0])
    seg_region_loss(z, m, bias=bias, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=0.25, grad_out=buf)              # and overwritten without
    assert torch.equal(buf, g["seg_logits"][:, 0])


@pytest.mark.parametrize("shape", SHAPES)
def test_autograd_node_hands_out_the_operator_gradient(shape):
    z, m = dev_inputs(shape)
    res, g = seg_region_loss(z, m, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=SMOOTH, with_grads=True)
    zz = z.clone().requires_grad_(True)
    total, dice, boundary = SegRegionLoss.apply(zz, m, W_DICE, W_BOUNDARY, SMOOTH)
    assert torch.equal(total, res[2]) and torch.equal(dice, res[0]) and torch.equal(boundary, res[1])
    assert total.requires_grad and not dice.requires_grad and not boundary.requires_grad
    (2.0 * total).backward()
    assert torch.equal(zz.grad, 2.0 * g["seg_logits"])


@pytest.mark.parametrize("shape", [(9, 63), (9, 65)])
def test_widths_next_to_a_word_boundary(shape):
    """W % 64 == 63 (and below 64) and W % 64 == 1: one padding bit, and one pixel in a word of its own; dense and packed targets."""
    z, m = dev_inputs(shape)
    ref = ref_of(shape, W_DICE, W_BOUNDARY)
    for mm, kw in ((m, {}), (pack_masks(m[:, 0]), dict(W=shape[1]))):
        res, g = seg_region_loss(z, mm, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, smooth=SMOOTH, with_grads=True, **kw)
        check_values(res, ref)
        check_grad(g["seg_logits"], ref[3])
