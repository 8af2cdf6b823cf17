"""`ValidationStep(det_loss="tal", instance_mask_weight=..., mask_assign="tal")`: a run trained with the task-aligned losses monitors
the loss it optimises.  The step equals the public operators called by hand on `vs.forward(x)`'s outputs (the same kernels in the same
order: `torch.equal`), `compute()` gains `val_epoch/loss_mask`, nothing synchronises, and the default construction returns what it
returned before.  The model and batch shape are those of tests/test_gpu_seg_tal_train.py (S = 128, B = 2)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, B = 128, 2
WEIGHTS = (1.0, 2.0, 1.5, 0.5, 1.0)

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, ValidationStep, instance_mask_loss, multitask_loss, task_aligned_det_loss)
    from oracle.model import ConvNeXtBiFPNYOLO as OModel, randomize_


def _model(seed=6):
    torch.manual_seed(seed)
    ora = randomize_(OModel(2, 2, pretrained_backbone=False), seed)
    hip = ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)
    hip.load_state_dict(ora.state_dict(), strict=True)
    return hip.to(DEV).train()


def _batch(seed=13):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, S, S, generator=g)
    gt_boxes = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 0, 0.4, 0.6, 0.5, 0.5], [1, 1, 0.3, 0.3, 0.2, 0.25]])
    gt_masks = torch.zeros(B, 1, S, S)
    gt_masks[0, 0, 45:83, 38:90] = 1
    gt_masks[1, 0, 45:109, 19:83] = 1
    return tuple(t.to(DEV) for t in (x, gt_boxes, gt_masks, torch.tensor([1, 0])))


def _by_hand(vs, proj, batch, *, det_loss, mask_w, mask_assign, iou_match_thresh=0.5):
    x, gt, masks, cls = batch
    det, (_, mc, protos), logits = vs.forward(x)
    w = WEIGHTS if det_loss == "reference" else (WEIGHTS[0], 0.0, 0.0, 0.0, WEIGHTS[4])
    ref = multitask_loss(det, protos, logits, gt, masks, cls, proj.weight, proj.bias, img_size=S, nc_det=2, training=False, weights=w,
                         iou_match_thresh=iou_match_thresh)
    out = tuple(ref)
    assigned = None
    if det_loss == "tal":
        r = task_aligned_det_loss(det, gt, img_size=S, nc_det=2, weights=WEIGHTS[1:4], want_assignment=mask_assign == "tal")
        tal = r[0] if mask_assign == "tal" else r
        assigned = r[1] if mask_assign == "tal" else None
        out = (ref[0] + (WEIGHTS[1] * tal[0] + WEIGHTS[2] * tal[1] + WEIGHTS[3] * tal[2]), ref[1], tal[0], tal[1], tal[2], ref[5])
    if mask_w > 0:
        m = instance_mask_loss(det, mc, protos, gt, masks, img_size=S, weight=mask_w, mc_layout="bnA", assigned=assigned,
                               iou_match_thresh=iou_match_thresh)
        out = (out[0] + mask_w * m[0],) + out[1:] + (m[0], m[1])
    return out


@pytest.mark.parametrize("det_loss,mask_w,mask_assign,thresh", [("tal", 1.0, "tal", 0.5), ("tal", 0.7, "iou", 0.05), ("reference", 0.7, "iou", 0.05),
                                                                ("tal", 0.0, "iou", 0.5)])
def test_validation_step_equals_the_public_operators_by_hand(det_loss, mask_w, mask_assign, thresh):
    model = _model()
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    batch = _batch()
    vs = ValidationStep(model, projector=proj, img_size=S, loss_weights=WEIGHTS, det_loss=det_loss, instance_mask_weight=mask_w,
                        mask_assign=mask_assign, iou_match_thresh=thresh)
    got = vs.step(*batch)
    assert model.training and all(m.training for m in model.modules())      # flags restored
    want = _by_hand(vs, proj, batch, det_loss=det_loss, mask_w=mask_w, mask_assign=mask_assign, iou_match_thresh=thresh)
    torch.cuda.synchronize()
    print(f"{det_loss} / {mask_w} / {mask_assign}: " + ", ".join(f"{float(v):.6f}" for v in got))
    assert len(got) == len(want) == (8 if mask_w > 0 else 6)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.isfinite(v) for v in got)
    if det_loss == "tal":
        assert float(got[2]) > 0 and float(got[3]) > 0 and float(got[4]) > 0
    if mask_assign == "tal":
        assert int(got[7]) > 0 and float(got[6]) > 0                       # the monitored mask term has positives
        r = task_aligned_det_loss(vs.forward(batch[0])[0], batch[1], img_size=S, nc_det=2)
        assert torch.equal(got[7], r[3])                                   # as many as there are foreground anchors
    logs = vs.compute()
    names = ("total", "seg", "box_iou", "dfl", "det_cls", "img_cls") + (("mask",) if mask_w > 0 else ())
    for name, v in zip(names, want):
        assert logs[f"val_epoch/loss_{name}"] == pytest.approx(float(v), rel=1e-12, abs=0), name
    assert ("val_epoch/loss_mask" in logs) == (mask_w > 0)
    assert isinstance(logs["val_epoch/det_confusion_matrix_epoch"], np.ndarray)


def test_the_tal_assignment_gives_the_mask_term_positives_where_the_iou_match_has_none():
    """A fresh model at `iou_match_thresh` 0.5: the reference's loss and the IoU-matched mask term say nothing, the task-aligned ones do."""
    model = _model()
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    batch = _batch()
    iou = ValidationStep(model, projector=proj, img_size=S, det_loss="tal", instance_mask_weight=1.0).step(*batch)
    tal = ValidationStep(model, projector=proj, img_size=S, det_loss="tal", instance_mask_weight=1.0, mask_assign="tal").step(*batch)
    assert int(iou[7]) == 0 and float(iou[6]) == 0.0
    assert int(tal[7]) > 0 and float(tal[6]) > 0
    assert all(torch.equal(a, b) for a, b in zip(iou[1:6], tal[1:6]))
    assert torch.equal(tal[0], iou[0] + 1.0 * tal[6])


def test_default_construction_returns_what_it_returned_before():
    model = _model()
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    batch = _batch()
    vs = ValidationStep(model, projector=proj, img_size=S)
    got = vs.step(*batch)
    x, gt, masks, cls = batch
    det, (_, _, protos), logits = vs.forward(x)
    ref = multitask_loss(det, protos, logits, gt, masks, cls, proj.weight, proj.bias, img_size=S, nc_det=2, training=False)
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(got, ref))
    explicit = ValidationStep(model, projector=proj, img_size=S, det_loss="reference", tal=None, instance_mask_weight=0.0, mask_assign="iou")
    got2 = explicit.step(*batch)
    assert len(got2) == 6 and all(torch.equal(a, b) for a, b in zip(got, got2))
    keys, keys2 = sorted(vs.compute()), sorted(explicit.compute())
    assert keys == keys2 and not any("mask" in k for k in keys)
    assert [k for k in keys if k.startswith("val_epoch/loss_")] == sorted(f"val_epoch/loss_{n}" for n in ("total", "seg", "box_iou", "dfl", "det_cls", "img_cls"))


def test_step_with_the_new_options_does_not_synchronise():
    model = _model()
    vs = ValidationStep(model, img_size=S, det_loss="tal", instance_mask_weight=1.0, mask_assign="tal")
    batch = _batch()
    vs.step(*batch)                                                        # warm-up: plans are built
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = vs.step(*batch)
        with pytest.raises(RuntimeError):                                  # positive control: the mode fires on this build
            losses[0].item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert np.isfinite(vs.compute()["val_epoch/loss_mask"])
