"""`TrainStep(instance_mask_weight=...)`: the instance-mask term wired into the native training step.  With the weight on, training
reaches Segment.cv4 (the mask coefficients) and the prototypes as a per-instance basis; at the default 0 nothing changes."""
import pytest
import torch

import mask_loss_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO
    from oracle import loss as oloss
    from oracle.model import ConvNeXtBiFPNYOLO as OModel, randomize_


def build(seed):
    """The oracle and the HIP model on one state_dict, both in train mode (as tests/test_gpu_train.py builds them)."""
    torch.manual_seed(seed)
    ora = randomize_(OModel(2, 2, pretrained_backbone=False), seed)
    hip = ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)
    hip.load_state_dict(ora.state_dict(), strict=True)
    hip = hip.to(DEV)
    ora.train()
    hip.train()
    return ora, hip


def _batch(S, B, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.rand(B, 3, S, S, generator=g) for _ in range(2)]
    gt_boxes = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 0, 0.4, 0.6, 0.5, 0.5], [1, 1, 0.3, 0.3, 0.2, 0.25]])
    gt_masks = torch.zeros(B, 1, S, S)
    gt_masks[0, 0, 45:83, 38:90] = 1
    gt_masks[1, 0, 45:109, 19:83] = 1
    return xs, gt_boxes, gt_masks, torch.tensor([1, 0])


def test_native_train_step_with_the_mask_term_matches_torch_loop_fp32():
    """tests/test_gpu_train.py::test_native_train_step_matches_torch_loop_fp32 with `instance_mask_weight = 0.7`: the torch side adds
    0.7 x the reference mask loss on the oracle's mc / protos outputs.  Two steps, SGD, clip 10, the same bounds."""
    W = 0.7
    ora, hip = build(6)
    S, B = 128, 2
    xs, gt_boxes, gt_masks, gt_cls = _batch(S, B, 13)
    proj = torch.nn.Conv2d(32, 1, 1)
    proj_h = torch.nn.Conv2d(32, 1, 1)
    proj_h.load_state_dict(proj.state_dict())
    kw = dict(iou_match_thresh=0.05, label_smoothing=0.1)
    before = {n: p.detach().clone() for n, p in ora.named_parameters()}
    lr, wd, mom = 0.05, 5e-4, 0.9
    opt = torch.optim.SGD(list(ora.parameters()) + list(proj.parameters()), lr=lr, momentum=mom, weight_decay=wd)
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=lr, weight_decay=wd, momentum=mom, clip_norm=10.0, projector=proj_h,
                   instance_mask_weight=W, **kw)
    assert ts.n_skip >= 1
    for step, x in enumerate(xs):
        opt.zero_grad(set_to_none=True)
        det_r, (_, mc_r, protos_r), logits_r = ora(x, "train")
        lr_ = oloss.multitask_loss(det_r, protos_r, logits_r, gt_boxes, gt_masks, gt_cls, proj.weight, proj.bias, img_size=S, nc_det=2, training=True, **kw)
        per_image = [p.numel() for p, _, _ in R.match(det_r, gt_boxes, S, 16, 0.05)]
        assert all(n > 0 for n in per_image), per_image                       # mask positives in both images
        ml, n_pos = R.mask_loss(det_r, mc_r.permute(0, 2, 1), protos_r, gt_boxes, gt_masks, img_size=S, reg_max=16, iou_match_thresh=0.05)
        total_r = lr_[0] + W * ml
        total_r.backward()
        total = torch.nn.utils.clip_grad_norm_(list(ora.parameters()) + list(proj.parameters()), 10.0)
        opt.step()
        lh = ts.step(x.to(DEV), gt_boxes.to(DEV), gt_masks.to(DEV), gt_cls.to(DEV))
        torch.cuda.synchronize()
        assert lh.shape == (10,)
        print(f"step {step}: total {lh[0].item():.6f} / {total_r.item():.6f}, mask {lh[8].item():.6f} / {ml.item():.6f}, positives {int(lh[9])} / {n_pos}, "
              f"norm {ts.gnorm.item():.6f} / {total.item():.6f}")
        assert abs(lh[0].item() - total_r.item()) <= 2e-3 * abs(total_r.item()), (step, lh[0].item(), total_r.item())
        assert abs(lh[8].item() - ml.item()) <= 2e-3 * abs(ml.item()), (step, lh[8].item(), ml.item())
        assert int(lh[9]) == n_pos
        assert abs(ts.gnorm.item() - total.item()) <= 2e-3 * total.item(), (step, ts.gnorm.item(), total.item())
    bad = []
    hp = dict(hip.named_parameters())
    ref_scale = max((p.detach() - before[n]).abs().max().item() for n, p in ora.named_parameters())
    for n, p in ora.named_parameters():
        want = p.detach() - before[n]
        got = hp[n].detach().float().cpu() - before[n]
        err = (got - want).abs().max().item()
        if err > 2e-3 * want.abs().max().item() + 1e-5 * ref_scale:
            bad.append(f"{n}: err {err:.3e} scale {want.abs().max().item():.3e}")
    assert not bad, f"{len(bad)} parameters moved differently:\n" + "\n".join(bad[:40])
    moved = lambda n: not torch.equal(hp[n].detach().cpu(), before[n])
    cv4 = [n for n in before if n.startswith("segment.cv4.") and n.endswith("weight")]
    assert cv4 and all(moved(n) for n in cv4)
    rest = [n for n in before if n.startswith(("segment.cv2.", "segment.cv3."))]
    assert rest and not any(moved(n) for n in rest)


def test_default_weight_leaves_the_step_as_it_was():
    _, hip = build(6)
    S, B = 128, 2
    xs, gt_boxes, gt_masks, gt_cls = _batch(S, B, 13)
    before = hip.state_dict()["segment.cv4.0.0.conv.weight"].detach().cpu().clone()
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.05, iou_match_thresh=0.05)
    assert ts.active == ("det", "logits", "protos")
    out = ts.step(xs[0].to(DEV), gt_boxes.to(DEV), gt_masks.to(DEV), gt_cls.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == (8,)
    assert torch.equal(dict(hip.named_parameters())["segment.cv4.0.0.conv.weight"].detach().cpu(), before)


def test_bf16_step_with_the_mask_term_is_finite_and_close_to_fp32():
    """One step at S = 128 with the weight on, bf16 storage: every gradient finite; the cv4 gradients point the way the fp32 step's do
    (the rule of tests/test_gpu_train.py::test_bf16_training_step_gradients_are_close_and_finite: cosine >= 0.9 for tensors of at
    least 64 elements that are not numerically zero -- but with no exceptions: its allowance of 8 is for a whole model's parameters,
    the cv4 branch has about two dozen)."""
    S, B = 128, 2
    xs, gt_boxes, gt_masks, gt_cls = _batch(S, B, 13)
    grads = {}
    for dt in (torch.float32, torch.bfloat16):
        _, hip = build(6)
        if dt != torch.float32:
            hip.set_compute_dtype(dt)
        ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.05, iou_match_thresh=0.05, instance_mask_weight=0.7)
        out = ts.forward_backward(xs[0].to(DEV), gt_boxes.to(DEV), gt_masks.to(DEV), gt_cls.to(DEV))
        torch.cuda.synchronize()
        assert out.shape == (10,) and torch.isfinite(out).all() and int(out[9]) > 0
        assert all(torch.isfinite(b).all() for b in ts.grads.buckets) and torch.isfinite(ts.pj_grad).all()
        grads[dt] = {n: v.detach().float().cpu().clone() for n, v in ts.grads.views.items() if n.startswith("segment.cv4.")}
    low, seen = [], 0
    for n, g32 in grads[torch.float32].items():
        g16 = grads[torch.bfloat16][n]
        assert g16.shape == g32.shape
        if g32.numel() < 64 or g32.abs().max().item() < 1e-6:
            continue
        seen += 1
        cos = torch.nn.functional.cosine_similarity(g16.double().flatten(), g32.double().flatten(), dim=0).item()
        print(f"{n}: cos {cos:.4f}")
        if cos < 0.9:
            low.append(f"{n}: cos {cos:.3f}")
    assert seen >= 12 and not low, "bf16 cv4 gradients diverge from the fp32 step:\n" + "\n".join(low)
