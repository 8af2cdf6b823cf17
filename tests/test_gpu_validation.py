"""The native validation step (validate.ValidationStep) and its two new device metrics: the detection confusion matrix of the eval-mode
loss (csrc/loss.hip `mtbt_det_confusion`) against a torch restatement of running_main_v3.py:298-350 written out here, the image-class
confusion matrix (csrc/metrics.hip `mtbt_cls_confusion`) against torch argmax, and the whole step against the same public functions
called by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, ValidationStep, init_synthetic_, multitask_loss, synthetic_images
    from multitask_bonetumor_yolo_amd.metrics import (DetectionConfusionMatrix, DeviceMeanAveragePrecision, ImageClassificationMetrics,
                                                      SegmentationMetrics)
    from multitask_bonetumor_yolo_amd.postprocess import decode_boxes, nms_batched, proto_projector_logits


# ---- torch restatement of the eval-mode loss's matched-anchor pairs (running_main_v3.py:298-350) -----------------------------
def _iou(b1, b2, eps=1e-7):
    x1 = torch.max(b1[:, 0].unsqueeze(1), b2[:, 0].unsqueeze(0))
    y1 = torch.max(b1[:, 1].unsqueeze(1), b2[:, 1].unsqueeze(0))
    x2 = torch.min(b1[:, 2].unsqueeze(1), b2[:, 2].unsqueeze(0))
    y2 = torch.min(b1[:, 3].unsqueeze(1), b2[:, 3].unsqueeze(0))
    inter = (x2 - x1).clamp(min=0) * (y2 - y1).clamp(min=0)
    a1 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1])
    a2 = (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    return inter / (a1.unsqueeze(1) + a2.unsqueeze(0) - inter + eps)


def torch_det_confusion(det, gt, S, nc, reg_max=16, thresh=0.5):
    """-> (counts [nc, nc] int64, every image's per-anchor max IoU): what `temp_matched_preds_for_cm` collects, counted."""
    boxes, logits = [], []
    proj = torch.arange(reg_max, dtype=torch.float32)
    for m in det:
        bs, ch, h, w = m.shape
        st = S / w
        f = m.permute(0, 2, 3, 1).reshape(bs, h * w, ch)
        dist = torch.einsum("ijkl,l->ijk", torch.softmax(f[..., : 4 * reg_max].view(bs, h * w, 4, reg_max), dim=-1), proj)
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        anc = torch.stack((gx + 0.5, gy + 0.5), -1).view(1, h * w, 2) * st
        d = dist * st
        boxes.append(torch.cat([anc - d[..., :2], anc + d[..., 2:]], -1))
        logits.append(f[..., 4 * reg_max:])
    boxes, logits = torch.cat(boxes, 1), torch.cat(logits, 1)
    counts = torch.zeros(nc, nc, dtype=torch.int64)
    max_ious = []
    for b in range(boxes.shape[0]):
        g = gt[gt[:, 0] == b]
        if g.numel() == 0:
            continue
        c = g[:, 2:6]
        gxy = torch.cat([(c[:, 0] - c[:, 2] / 2) * S, (c[:, 1] - c[:, 3] / 2) * S, (c[:, 0] + c[:, 2] / 2) * S, (c[:, 1] + c[:, 3] / 2) * S],
                        dim=-1).view(-1, 4)                                         # the reference's column concatenation (:303-308)
        v, idx = _iou(boxes[b], gxy).max(dim=1)
        max_ious.append(v)
        pos = v > thresh
        pred = logits[b][pos].argmax(dim=-1)
        tgt = g[:, 1].long()[idx[pos]]
        for t, p in zip(tgt.tolist(), pred.tolist()):
            counts[t, p] += 1
    return counts, torch.cat(max_ious)


def _det_case(nc, seed=3):
    """640 x 640, B = 4: image 0 holds two GT boxes (the column-concatenation quirk scrambles them), image 1 one, image 2 none, image 3
    three; anchors steered onto the (scrambled) boxes as tests/test_gpu_loss.py does, so that every image with GT has positives."""
    g = torch.Generator().manual_seed(seed)
    B, S = 4, 640
    det = [torch.randn(B, 64 + nc, h, h, generator=g) * 0.7 for h in (80, 40, 20)]
    gt = torch.tensor([[0, 1, 0.31, 0.36, 0.22, 0.30], [0, 0, 0.70, 0.70, 0.30, 0.25], [1, 0, 0.50, 0.50, 0.40, 0.35],
                       [3, 0, 0.25, 0.60, 0.30, 0.30], [3, nc - 1, 0.60, 0.30, 0.20, 0.40], [3, 1, 0.80, 0.80, 0.25, 0.25]])
    for lvl, h in enumerate((80, 40, 20)):
        stride = S / h
        for b in range(B):
            sel = gt[gt[:, 0] == b]
            if sel.numel() == 0:
                continue
            c = sel[:, 2:6]
            boxes = torch.cat([(c[:, 0] - c[:, 2] / 2) * S, (c[:, 1] - c[:, 3] / 2) * S, (c[:, 0] + c[:, 2] / 2) * S,
                               (c[:, 1] + c[:, 3] / 2) * S], dim=-1).view(-1, 4)
            for bx in boxes:
                if bx[2] <= bx[0] or bx[3] <= bx[1]:
                    continue
                cx, cy = int((bx[0] + bx[2]) / 2 / stride), int((bx[1] + bx[3]) / 2 / stride)
                for yy in range(max(cy - 1, 0), min(cy + 2, h)):
                    for xx in range(max(cx - 1, 0), min(cx + 2, h)):
                        ax, ay = (xx + 0.5) * stride, (yy + 0.5) * stride
                        ltrb = torch.tensor([ax - bx[0], ay - bx[1], bx[2] - ax, bx[3] - ay]) / stride
                        if ltrb.min() > 0.3 and ltrb.max() < 14.0:
                            for k in range(4):
                                det[lvl][b, 16 * k:16 * k + 16, yy, xx] += 6.0 * torch.exp(-0.5 * (torch.arange(16.0) - ltrb[k]) ** 2 / 0.3)
    return det, gt, S


@pytest.mark.parametrize("nc", [2, 3])
def test_det_confusion_matches_torch_restatement(nc):
    det, gt, S = _det_case(nc)
    want, max_iou = torch_det_confusion(det, gt, S, nc)
    margin = (max_iou - 0.5).abs().min().item()
    assert margin > 1e-5, f"an anchor's max IoU lies {margin} from the threshold: exact equality would hinge on the last ulp"
    assert want.sum() > 20 and (want.sum(1) > 0).sum() >= 2             # positives in several images and target classes
    m = DetectionConfusionMatrix(nc, S)
    dd = [d.to(DEV) for d in det]
    m.update(dd, gt.to(DEV))
    got = m.compute()
    assert np.array_equal(got["confusion_counts"], want.numpy()), (got["confusion_counts"], want)
    rows = want.sum(1, keepdim=True).double()
    assert np.allclose(got["confusion_matrix"], torch.where(rows > 0, want / rows.clamp(min=1), 0.0).numpy(), rtol=0, atol=1e-15)
    # its positives are the loss's positives
    protos = torch.randn(4, 32, 160, 160, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = multitask_loss(dd, protos, torch.randn(4, 2).to(DEV), gt.to(DEV), torch.zeros(4, 1, S, S, device=DEV), torch.zeros(4, dtype=torch.long, device=DEV),
                         torch.randn(1, 32, 1, 1).to(DEV), torch.zeros(1, device=DEV), img_size=S, nc_det=nc, training=True)
    assert int(got["confusion_counts"].sum()) == int(out[6].item())
    # counts accumulate across calls; channels-last maps give the same counts
    m.update([d.contiguous(memory_format=torch.channels_last) for d in dd], gt.to(DEV))
    assert np.array_equal(m.compute()["confusion_counts"], 2 * want.numpy())


def test_image_counts_match_argmax_with_ties_and_nan():
    g = torch.Generator().manual_seed(5)
    N, nc = 3000, 4
    logits = torch.randint(-2, 3, (N, nc), generator=g).float()        # small integers: many tied maxima
    logits[7, 2] = float("nan")
    logits[8, 0] = float("nan")
    logits[9, 1] = logits[9, 3] = float("nan")
    target = torch.randint(0, nc, (N,), generator=g)
    x, t = logits.to(DEV), target.to(DEV)
    m = ImageClassificationMetrics(nc)
    m.update(x[:1000], t[:1000])
    m.update(x[1000:], t[1000:])
    got = m.compute()
    pred = x.argmax(dim=-1).cpu()
    assert pred[7] == 2 and pred[8] == 0 and pred[9] == 1                 # torch: a NaN is the maximum, the first one wins
    want = torch.zeros(nc, nc, dtype=torch.int64)
    want.index_put_((target, pred), torch.ones(N, dtype=torch.int64), accumulate=True)
    assert np.array_equal(got["confusion_counts"], want.numpy())
    assert got["accuracy"] == float((pred == target).sum()) / N


def test_out_of_range_classes_raise():
    det, gt, S = _det_case(2)
    bad = gt.clone()
    bad[2, 1] = 2                                                          # image 1's box: class 2 of nc = 2
    m = DetectionConfusionMatrix(2, S)
    m.update([d.to(DEV) for d in det], bad.to(DEV))
    with pytest.raises(ValueError):
        m.compute()
    m.reset()
    m.update([d.to(DEV) for d in det], gt.to(DEV))
    assert m.compute()["confusion_counts"].sum() > 0
    c = ImageClassificationMetrics(3)
    c.update(torch.randn(4, 3, device=DEV), torch.tensor([0, 1, 3, 2], device=DEV))
    with pytest.raises(ValueError):
        c.compute()


def test_cpu_tensors_are_rejected():
    with pytest.raises(RuntimeError):
        ImageClassificationMetrics(2).update(torch.randn(4, 2), torch.zeros(4, dtype=torch.long))
    det, gt, S = _det_case(2)
    with pytest.raises(RuntimeError):
        DetectionConfusionMatrix(2, S).update(det, gt)
    vs = ValidationStep(_model(), img_size=128)
    with pytest.raises(RuntimeError):
        vs.step(*_batch(2, 128, 0, dev="cpu"))


# ---- the whole step ---------------------------------------------------------------------------------------------------------
def _model():
    torch.manual_seed(0)
    return init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV)


def _batch(B, S, seed, dev=DEV):
    g = torch.Generator().manual_seed(100 + seed)
    imgs = synthetic_images(B, S, seed=seed)
    rows = []
    for b in range(B):
        for _ in range(b % 3):
            wh = torch.rand(2, generator=g) * 0.3 + 0.1
            cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            rows.append(torch.cat([torch.tensor([float(b), float(torch.randint(0, 2, (1,), generator=g))]), cxy, wh]))
    gt = torch.stack(rows) if rows else torch.zeros(0, 6)
    masks = (torch.rand(B, 1, S, S, generator=g) > 0.7).float()
    cls = torch.randint(0, 2, (B,), generator=g)
    return imgs.to(dev), gt.to(dev), masks.to(dev), cls.to(dev)


def test_validation_step_equals_the_public_functions_by_hand():
    model = _model()
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    S = 128
    batches = [_batch(4, S, 1), _batch(2, S, 2)]
    model.train()
    vs = ValidationStep(model, projector=proj, img_size=S)
    losses = [vs.step(*b) for b in batches]
    assert model.training and all(m.training for m in model.modules())      # flags restored
    got = vs.compute()

    seg, img, dcm = SegmentationMetrics(), ImageClassificationMetrics(2), DetectionConfusionMatrix(2, S)
    m50, m5095 = DeviceMeanAveragePrecision([0.5], (1, 10, 100)), DeviceMeanAveragePrecision(None, (1, 10, 100))
    sums, n = np.zeros(6), 0
    for (x, gt, masks, cls), lv in zip(batches, losses):
        model.eval()
        with torch.no_grad():
            det, (_, _, protos), logits = model(x, "train")
        model.train()
        ref = multitask_loss(det, protos, logits, gt, masks, cls, proj.weight, proj.bias, img_size=S, nc_det=2, training=False)
        assert len(lv) == 6 and all(torch.equal(a, b) for a, b in zip(lv, ref))
        sums += np.array([float(v) for v in ref], np.float64) * x.shape[0]
        n += x.shape[0]
        seg.update(proto_projector_logits(protos, proj.weight, proj.bias, S), masks)
        img.update(logits, cls)
        dcm.update(det, gt)
        d = decode_boxes(det, S, want_scores=False)
        k = nms_batched(d["boxes"], d["best_score"], d["best_label"], float(S), 0.05, 0.6, 100)
        m50.update_batched(k, gt, S)
        m5095.update_batched(k, gt, S)
    want = {f"val_epoch/loss_{k}": v for k, v in zip(("total", "seg", "box_iou", "dfl", "det_cls", "img_cls"), sums / n)}
    ic = img.compute()
    want.update({"val_epoch/img_accuracy_epoch": ic["accuracy"], "val_epoch/img_confusion_matrix_epoch": ic["confusion_matrix"],
                 "val_epoch/img_precision_macro": ic["precision_macro"], "val_epoch/img_recall_macro": ic["recall_macro"],
                 "val_epoch/img_f1_macro": ic["f1_macro"], "val_epoch/det_confusion_matrix_epoch": dcm.compute()["confusion_matrix"]})
    sc = seg.compute()
    want.update({f"val_epoch/seg_{k}_epoch": sc[k] for k in ("f1", "precision", "recall", "accuracy", "dice")})
    want.update({f"val_epoch/seg_map_{k}": v for k, v in seg.compute_map().items()})
    want.update({f"val_epoch/map_iou50_{k}": v for k, v in m50.compute().items()})
    want.update({f"val_epoch/map_iou50_95_{k}": v for k, v in m5095.compute().items()})
    want["val_epoch_map_iou50/map"] = want["val_epoch/map_iou50_map"]
    assert sorted(got) == sorted(want)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), k
        else:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), (k, got[k], want[k])
    for k in ("map", "map_50", "map_75", "map_small", "mar_100", "mar_large"):
        assert f"val_epoch/seg_map_{k}" in got and f"val_epoch/map_iou50_95_{k}" in got
    vs.reset()
    assert vs.compute()["val_epoch/loss_total"] == 0.0


def test_step_does_not_synchronise():
    model = _model()
    S = 128
    vs = ValidationStep(model, img_size=S)
    batch = _batch(4, S, 3)
    vs.step(*batch)                                                        # warm-up: plans are built
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = vs.step(*batch)
        with pytest.raises(RuntimeError):                                  # positive control: the mode fires on this build
            losses[0].item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert np.isfinite(vs.compute()["val_epoch/loss_total"])
