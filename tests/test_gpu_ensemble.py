"""Test-time augmentation and ensembles (ensemble.detect_fused, ValidationStep(views=...)) on a synthetic model at S = 128: the fused
route against the same public functions called by hand and the numpy restatement of the fusion (tests/fuse_reference.py)."""
import numpy as np
import pytest
import torch

from fuse_reference import fuse_detections as ref_fuse

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, B, TOP_K = 128, 3, 50
NMS = dict(conf_th=0.05, iou_th=0.6, top_k=TOP_K)

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, ValidationStep, calibrate_synthetic_heads_, detect_fused, init_synthetic_,
                                              synthetic_images)
    from multitask_bonetumor_yolo_amd.postprocess import assemble_masks, detect_and_segment, orient_batch, unorient_batch

KEYS = ("boxes", "scores", "labels", "counts", "n_clusters", "n_members", "lead_source", "lead_slot", "lead_anchor")


def _model(seed):
    torch.manual_seed(seed)
    m = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=seed).to(DEV).eval()
    return calibrate_synthetic_heads_(m, synthetic_images(B, S, seed=5).to(DEV))


@pytest.fixture(scope="module")
def models():
    return _model(0), _model(1)


@pytest.fixture(scope="module")
def x():
    return synthetic_images(B, S, seed=5).to(DEV)


def _source(model, x, view):
    """One source by hand: the view, the model, the post-process."""
    with torch.no_grad():
        out = model(orient_batch(x, view), "infer")
    _, mc, protos = out["segment_protos"]
    return out, detect_and_segment(out["detect_features"], mc, protos, S, masks=False, **NMS)


def _numpy(d):
    return {"boxes": d["boxes"].cpu().numpy(), "scores": d["scores"].cpu().numpy(), "labels": d["labels"].cpu().numpy(),
            "counts": d["counts"].cpu().numpy(), "keep_anchor": d["keep_anchor"].cpu().numpy()}


def _equal(got, want):
    for k in KEYS:
        g, w = got[k].cpu(), torch.from_numpy(np.asarray(want[k]))
        assert g.dtype == w.dtype and torch.equal(g, w), k


def test_orient_batch_is_the_pixel_rule_and_has_an_inverse(x):
    for o in range(8):
        q = orient_batch(x, o)
        t = x.transpose(2, 3) if o & 4 else x
        t = t.flip(3) if o & 1 else t
        t = t.flip(2) if o & 2 else t
        assert torch.equal(q, t) and torch.equal(unorient_batch(q, o), x)
    with pytest.raises(ValueError):
        orient_batch(x[:, :, :, :64], 1)


def test_identity_route_is_detect_and_segment(models, x):
    _, d = _source(models[0], x, 0)
    assert int(d["counts"].min()) > 0
    got = detect_fused(models[0], x, S, views=(0,), wbf_iou=1.0, **NMS)
    for k in ("boxes", "scores", "labels", "counts"):
        assert torch.equal(got[k], d[k]), k
    assert torch.equal(got["lead_anchor"], d["keep_anchor"])


def test_two_views_equal_fusing_by_hand(models, x):
    dets = [_source(models[0], x, v)[1] for v in (0, 1)]
    want = ref_fuse([_numpy(d) for d in dets], S, orients=[0, 1], top_k=TOP_K)
    assert (want["n_members"] >= 2).any()
    _equal(detect_fused(models[0], x, S, views=(0, 1), **NMS), want)


def test_ensemble_of_two_models_with_weights(models, x):
    dets = [_source(m, x, v)[1] for m in models for v in (0, 6)]
    want = ref_fuse([_numpy(d) for d in dets], S, orients=[0, 6, 0, 6], weights=[1.0, 1.0, 2.0, 2.0], top_k=TOP_K)
    assert len(set(want["lead_source"][want["lead_source"] >= 0].tolist())) > 1
    _equal(detect_fused(list(models), x, S, views=(0, 6), weights=(1.0, 2.0), **NMS), want)


def test_masks_are_the_leaders_planes_turned_back(models, x):
    views = (0, 5)
    got = detect_fused(models[0], x, S, views=views, masks=True, **NMS)
    assert got["masks"].dtype == torch.uint8 and tuple(got["masks"].shape) == (B, TOP_K, S, S)
    planes = []
    for v in views:
        out, d = _source(models[0], x, v)
        _, mc, protos = out["segment_protos"]
        m, _ = assemble_masks(protos, mc.float(), d["keep_anchor"], d["counts"], (S, S))
        planes.append(unorient_batch(m.view(torch.uint8), v))
    ls, lk, cnt = got["lead_source"].cpu(), got["lead_slot"].cpu(), got["counts"].cpu()
    assert set(ls[ls >= 0].tolist()) == {0, 1} and got["masks"].any()
    for b in range(B):
        for r in range(TOP_K):
            want = planes[ls[b, r]][b, lk[b, r]] if r < cnt[b] else torch.zeros_like(got["masks"][b, r])
            assert torch.equal(got["masks"][b, r], want), (b, r)


def _batch(seed):
    g = torch.Generator().manual_seed(100 + seed)
    rows = []
    for b in range(B):
        for _ in range(1 + b % 2):
            wh = torch.rand(2, generator=g) * 0.3 + 0.1
            cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            rows.append(torch.cat([torch.tensor([float(b), float(torch.randint(0, 2, (1,), generator=g))]), cxy, wh]))
    masks = (torch.rand(B, 1, S, S, generator=g) > 0.7).float()
    return synthetic_images(B, S, seed=seed).to(DEV), torch.stack(rows).to(DEV), masks.to(DEV), torch.randint(0, 2, (B,), generator=g).to(DEV)


def test_validation_step_views(models):
    model = models[0]
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    batch = _batch(5)
    plain = ValidationStep(model, projector=proj, img_size=S)
    same = ValidationStep(model, projector=proj, img_size=S, views=(0,), wbf_iou=1.0)
    tta = ValidationStep(model, projector=proj, img_size=S, views=(0, 1))
    lp, ls, lt = plain.step(*batch), same.step(*batch), tta.step(*batch)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(lp, ls, lt))          # the losses stay on the identity pass
    cp, cs, ct = plain.compute(), same.compute(), tta.compute()
    assert sorted(cp) == sorted(cs) == sorted(ct)
    for k in cp:
        if "map_iou50" in k:
            assert cs[k] == cp[k], k                                                             # one view, IoU 1.0: the same detections
        elif isinstance(cp[k], np.ndarray):
            assert np.array_equal(ct[k], cp[k]), k                                               # everything else never sees the views
        else:
            assert ct[k] == cp[k] or (np.isnan(ct[k]) and np.isnan(cp[k])), k
    assert not model.training
    with pytest.raises(NotImplementedError, match="detect_fused"):
        ValidationStep(model, projector=proj, img_size=S, views=(0, 1), instance_masks=True)
