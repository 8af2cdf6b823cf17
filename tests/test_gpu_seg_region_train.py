"""`TrainStep(seg_dice_weight=, seg_boundary_weight=)`: the region terms of `seg_region_loss` inside the native training step.  At
weights 0 (the default) nothing changes, bit for bit; with a weight > 0 the total gains the weighted sum, two elements are appended,
and the region gradient reaches the projector through `dseg`.  Batch shape, model and batch of tests/test_gpu_seg_tal_train.py; every
configuration gets a model of its own from the same seed."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, B = 128, 2
W_DICE, W_BOUNDARY = 1.0, 0.01

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, TrainStep, multitask_loss, seg_region_loss
    from oracle.model import ConvNeXtBiFPNYOLO as OModel, randomize_


def make(**kw):
    """A TrainStep over the model of tests/test_gpu_seg_tal_train.py (the oracle's state_dict, seed 6) and a projector from the same seed."""
    torch.manual_seed(6)
    hip = ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)
    hip.load_state_dict(randomize_(OModel(2, 2, pretrained_backbone=False), 6).state_dict(), strict=True)
    hip = hip.to(DEV).train()
    torch.manual_seed(7)
    proj = torch.nn.Conv2d(hip.proto_ch, 1, 1)
    return TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.01, iou_match_thresh=0.05, projector=proj, **kw)


def batch():
    g = torch.Generator().manual_seed(13)
    x = torch.rand(B, 3, S, S, generator=g)
    gt_boxes = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 0, 0.4, 0.6, 0.5, 0.5], [1, 1, 0.3, 0.3, 0.2, 0.25]])
    gt_masks = torch.zeros(B, 1, S, S)
    gt_masks[0, 0, 45:83, 38:90] = 1
    gt_masks[1, 0, 45:109, 19:83] = 1
    return tuple(t.to(DEV) for t in (x, gt_boxes, gt_masks, torch.tensor([1, 0])))


_RUNS = {}


def runs():
    """One `forward_backward` per configuration on identically seeded models, shared by the tests: (TrainStep, result, pj_grad copy)."""
    if not _RUNS:
        for name, kw in (("plain", {}), ("zero", dict(seg_dice_weight=0.0, seg_boundary_weight=0.0, seg_dice_smooth=1.0)),
                         ("on", dict(seg_dice_weight=W_DICE, seg_boundary_weight=W_BOUNDARY))):
            ts = make(**kw)
            out = ts.forward_backward(*batch())
            torch.cuda.synchronize()
            _RUNS[name] = (ts, out.clone(), ts.pj_grad.clone())
    return _RUNS


def test_at_zero_weights_nothing_changes():
    r = runs()
    (_, plain, pj_plain), (_, zero, pj_zero) = r["plain"], r["zero"]
    assert plain.shape == zero.shape == (8,) and torch.isfinite(plain).all()
    assert torch.equal(plain, zero) and torch.equal(pj_plain, pj_zero)


def test_the_terms_reach_the_total_the_tuple_and_the_projector():
    r = runs()
    (off, plain, pj_plain), (ts, on, pj_on) = r["plain"], r["on"]
    assert on.shape == (10,) and torch.isfinite(on).all()
    assert torch.equal(on[1:8], plain[1:8])                                   # the reference's terms do not move
    dice, boundary = float(on[8]), float(on[9])
    assert 0.0 < dice < 1.0 and boundary != 0.0
    weighted = W_DICE * dice + W_BOUNDARY * boundary
    print("total off / on", float(plain[0]), float(on[0]), "dice", dice, "boundary", boundary)
    # one fp32 addition of two fp32 numbers of the totals' size: rtol 1e-5 (the operator's value tolerance) of the larger
    assert float(on[0]) - float(plain[0]) == pytest.approx(weighted, abs=1e-5 * max(abs(float(on[0])), abs(weighted)))
    # the operator on the bias-free logits of the same forward (same weights, same batch: `off` has not been stepped)
    x, gt_boxes, gt_masks, gt_cls = batch()
    off.tp.run_forward(x)
    _, seg_logits = multitask_loss([m.nchw() for m in off.tp.det_maps], off.tp.protos.nchw(), off.tp.logits, gt_boxes, gt_masks, gt_cls,
                                   off.projector.weight, off.projector.bias, want_seg_logits=True, **off.loss_kw)
    assert tuple(seg_logits.shape) == (B, 1, S, S)
    res, g = seg_region_loss(seg_logits, gt_masks, bias=off.projector.bias, dice_weight=W_DICE, boundary_weight=W_BOUNDARY, with_grads=True)
    assert torch.equal(res[0], on[8]) and torch.equal(res[1], on[9])
    # the projector bias gradient moved by the sum of the operator's gradient: the operator test's tolerances, the absolute one scaled
    # from one element to a sum (1e-6 * sum |d| in place of 1e-6 * max |d|)
    nm = ts.m.proto_ch
    d = g["seg_logits"].double()
    moved, want = float(pj_on[nm]) - float(pj_plain[nm]), float(d.sum())
    print("bias gradient off / on", float(pj_plain[nm]), float(pj_on[nm]), "moved", moved, "sum d_logits", want)
    assert want != 0.0 and abs(moved - want) <= 1e-4 * abs(want) + 1e-6 * float(d.abs().sum())
    assert not torch.equal(pj_on[:nm], pj_plain[:nm])                         # and the weight gradient with it


def test_the_weights_are_attributes_and_a_second_step_stays_finite():
    ts = make(seg_dice_weight=W_DICE, seg_boundary_weight=0.0)
    b = batch()
    first = ts.step(*b)
    assert first.shape == (10,) and float(first[9]) == 0.0                    # no boundary term yet
    ts.seg_boundary_weight = W_BOUNDARY                                       # Kervadec's schedule: an assignment between steps
    second = ts.step(*b)
    torch.cuda.synchronize()
    assert second.shape == (10,) and float(second[9]) != 0.0 and torch.isfinite(second).all()
    assert all(torch.isfinite(p).all() for p in ts.params.buckets) and torch.isfinite(ts.pj).all()
    sd = ts.state_dict()
    assert sd["seg_dice_weight"] == W_DICE and sd["seg_boundary_weight"] == W_BOUNDARY and sd["seg_dice_smooth"] == 1.0
    legacy = {k: v for k, v in sd.items() if not k.startswith("seg_")}        # a state from before the keys loads as before
    ts.load_state_dict(legacy)
    ts.seg_dice_weight = ts.seg_boundary_weight = 0.0
    assert ts.step(*b).shape == (8,)
