"""`TrainStep(det_loss="tal", instance_mask_weight=..., mask_assign="tal")`: the instance-mask term driven by the task-aligned
assignment inside the native training step.  A freshly initialised model's mask branch gets a gradient from it where the mask loss's
own IoU match (positives need a predicted box with IoU > 0.5) gives it none; at the default "iou" nothing changes.  The model and the
batch are those of tests/test_gpu_tal_train.py (model seed 6, batch seed 13)."""
import pytest
import torch

import seg_tal_reference as R
import tal_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, B = 128, 2

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, load_train_state, save_train_state
    from oracle import loss as oloss
    from oracle.model import ConvNeXtBiFPNYOLO as OModel, randomize_


def build(seed):
    """The oracle and the HIP model on one state_dict, both in train mode (as tests/test_gpu_train.py builds them): default inits."""
    torch.manual_seed(seed)
    ora = randomize_(OModel(2, 2, pretrained_backbone=False), seed)
    hip = ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)
    hip.load_state_dict(ora.state_dict(), strict=True)
    hip = hip.to(DEV)
    ora.train()
    hip.train()
    return ora, hip


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.rand(B, 3, S, S, generator=g) for _ in range(2)]
    gt_boxes = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 0, 0.4, 0.6, 0.5, 0.5], [1, 1, 0.3, 0.3, 0.2, 0.25]])
    gt_masks = torch.zeros(B, 1, S, S)
    gt_masks[0, 0, 45:83, 38:90] = 1
    gt_masks[1, 0, 45:109, 19:83] = 1
    return xs, gt_boxes, gt_masks, torch.tensor([1, 0])


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


_FRESH = {}


def _fresh(mode, topk=10):
    """One `forward_backward` of a default-initialised model per (mask assignment, topk), shared by the two tests below: (the 10-element
    result, the cv4 gradients by parameter name, whether d_mc has a non-zero entry, anchors with a d_mc row per level)."""
    if (mode, topk) not in _FRESH:
        xs, gt_boxes, gt_masks, gt_cls = _batch(13)
        _, hip = build(6)
        ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.05, det_loss="tal", tal=dict(topk=topk), instance_mask_weight=1.0,
                       mask_assign=mode)                                                        # iou_match_thresh at its default 0.5
        out = ts.forward_backward(*_dev(xs[0], gt_boxes, gt_masks, gt_cls))
        torch.cuda.synchronize()
        assert out.shape == (10,) and torch.isfinite(out).all()
        gr = {n: v.detach().float().cpu() for n, v in ts.grads.views.items() if n.startswith("segment.cv4.")}
        d_mc = ts.tp.d_in["mc"].view(B, -1, 32)
        sizes = [(S // st) ** 2 for st in (8, 16, 32)]
        per_level = [int(d.any(-1).sum()) for d in d_mc.split(sizes, dim=1)]
        _FRESH[(mode, topk)] = (out.cpu(), gr, bool(d_mc.any()), per_level)
        print(f"mask_assign={mode} topk={topk}: foreground anchors {int(out[6])}, mask positives {int(out[9])}, mask loss {out[8].item():.6f}, "
              f"anchors with a d_mc row per level {per_level}")
    return _FRESH[(mode, topk)]


def test_every_cv4_weight_gradient_of_a_fresh_model_is_non_zero():
    """Default-initialised heads, `iou_match_thresh` at its default 0.5, one `forward_backward` per configuration.  With
    `det_loss="tal", instance_mask_weight=1.0` the mask term has 0 positives and `segment.cv4` gets an exactly zero gradient; adding
    `mask_assign="tal"` gives slot 9 == slot 6 > 0 and EVERY `segment.cv4.*weight` gradient is non-zero.
    The assigner runs at topk = 64 here, its maximum: cv4 is one branch per level and a branch sees the loss only through foreground
    anchors of its level, so "every weight" needs foreground anchors on all three.  At topk 64 this model and batch (seeds 6 / 13) have
    97 / 10 / 5 of them on the stride-8 / 16 / 32 levels (`tal_reference.assign` on the oracle's maps; autograd through the oracle then
    gives max |gradient| between 2.6e-3 and 0.15 on all fifteen weights).  At the default topk 10 all 30 lie on the stride-8 level and
    the two other branches get exact zeros from any correct implementation: that configuration is the next test."""
    out_i, gr_i, any_i, _ = _fresh("iou", 64)
    assert int(out_i[6]) > 0 and int(out_i[9]) == 0 and float(out_i[8]) == 0.0 and not any_i
    assert gr_i and not any(g.any() for g in gr_i.values())           # cv4 gets exactly nothing
    out_t, gr_t, any_t, per_level = _fresh("tal", 64)
    assert int(out_t[9]) == int(out_t[6]) == int(out_i[6]) > 0 and float(out_t[8]) > 0 and any_t
    assert sum(per_level) == int(out_t[6]) and all(n > 0 for n in per_level)
    weights = [n for n in gr_t if n.endswith("weight")]
    zero = [n for n in weights if not gr_t[n].abs().max().item() > 0]
    print(f"foreground anchors per level {per_level}; cv4 weights with an exactly zero gradient: {zero}")
    assert len(weights) == 15 and not zero
    assert torch.equal(out_t[1:8], out_i[1:8])                        # the other terms do not depend on the mask assignment


def test_at_the_default_topk_a_level_without_foreground_anchors_gets_exact_zeros():
    """The same at the default topk 10: 0 mask positives and an exactly zero cv4 gradient with the IoU match; with the assignment as many
    positives as foreground anchors, a non-zero gradient on every weight of the cv4 branch of each level that holds one, and exact zeros
    on a level WITHOUT one -- as background anchors get, and as autograd through the oracle gives (all 30 lie on the stride-8 level)."""
    out_i, gr_i, any_i, _ = _fresh("iou")
    assert int(out_i[6]) > 0 and int(out_i[9]) == 0 and float(out_i[8]) == 0.0 and not any_i
    assert gr_i and not any(g.any() for g in gr_i.values())
    out_t, gr_t, any_t, per_level = _fresh("tal")
    assert int(out_t[9]) == int(out_t[6]) == int(out_i[6]) > 0 and float(out_t[8]) > 0 and any_t
    assert sum(per_level) == int(out_t[6]) and per_level[0] > 0
    assert torch.equal(out_t[1:8], out_i[1:8])
    for lvl, n in enumerate(per_level):
        names = [k for k in gr_t if k.startswith(f"segment.cv4.{lvl}.") and k.endswith("weight")]
        assert names
        if n > 0:
            assert all(gr_t[k].abs().max().item() > 0 for k in names), lvl
        else:
            assert not any(gr_t[k].any() for k in gr_t if k.startswith(f"segment.cv4.{lvl}.")), lvl


def test_native_train_step_with_the_assigned_mask_term_matches_torch_loop_fp32():
    """tests/test_gpu_tal_train.py::test_native_train_step_with_the_tal_loss_matches_torch_loop_fp32 with `w_mask *
    seg_tal_reference.mask_loss_from_assignment` added on the oracle's mc / protos outputs, on `tal_reference.assign` of the oracle's
    maps.  Two steps, SGD, clip 10, the same bounds; n_fg equal in both steps.  The second step's assignment depends on weights the mask
    term has moved: with batch seed 13 the oracle loop alone has margins (relative metric gap, contested-overlap gap) of (8.6e-3, none
    contested) at step 1 and (3.0e-3, none contested) at step 2, checked on the CPU and asserted again below (>= 1e-4), so the batch
    seed of that test is kept."""
    W = 1.0
    ora, hip = build(6)
    xs, gt_boxes, gt_masks, gt_cls = _batch(13)
    proj = torch.nn.Conv2d(32, 1, 1)
    proj_h = torch.nn.Conv2d(32, 1, 1)
    proj_h.load_state_dict(proj.state_dict())
    weights = (1.0, 2.0, 1.5, 0.5, 1.0)
    before = {n: p.detach().clone() for n, p in ora.named_parameters()}
    lr, wd, mom = 0.05, 5e-4, 0.9
    opt = torch.optim.SGD(list(ora.parameters()) + list(proj.parameters()), lr=lr, momentum=mom, weight_decay=wd)
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=lr, weight_decay=wd, momentum=mom, clip_norm=10.0, projector=proj_h,
                   label_smoothing=0.1, loss_weights=weights, det_loss="tal", instance_mask_weight=W, mask_assign="tal")
    for step, x in enumerate(xs):
        opt.zero_grad(set_to_none=True)
        det_r, (_, mc_r, protos_r), logits_r = ora(x, "train")
        lr_ = oloss.multitask_loss(det_r, protos_r, logits_r, gt_boxes, gt_masks, gt_cls, proj.weight, proj.bias, img_size=S, nc_det=2, training=True,
                                   label_smoothing=0.1, weights=(weights[0], 0.0, 0.0, 0.0, weights[4]))
        asg = T.assign(det_r, gt_boxes, img_size=S)
        tight_m, tight_o = R.margins(asg, 10)
        box, dfl, cls, n_fg, mov = T.tal_loss(det_r, gt_boxes, img_size=S, asg=asg)
        ml, n_mask = R.mask_loss_from_assignment(mc_r.permute(0, 2, 1), protos_r, gt_boxes, gt_masks, asg["assigned"], asg["off"], img_size=S)
        total_r = lr_[0] + weights[1] * box + weights[2] * dfl + weights[3] * cls + W * ml
        total_r.backward()
        total = torch.nn.utils.clip_grad_norm_(list(ora.parameters()) + list(proj.parameters()), 10.0)
        opt.step()
        lh = ts.step(*_dev(x, gt_boxes, gt_masks, gt_cls))
        torch.cuda.synchronize()
        assert lh.shape == (10,)
        print(f"step {step}: margins {tight_m:.3e} / {tight_o:.3e}, total {lh[0].item():.6f} / {total_r.item():.6f}, box {lh[2].item():.6f} / "
              f"{box.item():.6f}, dfl {lh[3].item():.6f} / {dfl.item():.6f}, cls {lh[4].item():.6f} / {cls.item():.6f}, mask {lh[8].item():.6f} / "
              f"{ml.item():.6f}, fg {int(lh[6])} / {int(lh[9])} / {n_fg}, norm {ts.gnorm.item():.6f} / {total.item():.6f}")
        assert tight_m >= 1e-4 and tight_o >= 1e-4
        assert n_fg > 0 and n_mask == n_fg and int(lh[6]) == n_fg and int(lh[9]) == n_fg
        assert abs(lh[0].item() - total_r.item()) <= 2e-3 * abs(total_r.item()), (step, lh[0].item(), total_r.item())
        for i, want in ((2, box), (3, dfl), (4, cls), (8, ml)):
            assert abs(lh[i].item() - want.item()) <= 2e-3 * abs(want.item()), (step, i, lh[i].item(), want.item())
        assert abs(lh[7].item() - mov) <= 2e-3 * abs(mov)
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
    heads = [n for n in before if n.startswith(("detect.cv2.", "detect.cv3.", "segment.cv4.")) and n.endswith("weight")]
    assert heads and all(moved(n) for n in heads)
    rest = [n for n in before if n.startswith(("segment.cv2.", "segment.cv3."))]
    assert rest and not any(moved(n) for n in rest)


def test_bf16_step_with_the_assigned_mask_term_is_finite():
    xs, gt_boxes, gt_masks, gt_cls = _batch(13)
    _, hip = build(6)
    hip.set_compute_dtype(torch.bfloat16)
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.05, det_loss="tal", instance_mask_weight=1.0, mask_assign="tal")
    out = ts.step(*_dev(xs[0], gt_boxes, gt_masks, gt_cls))
    torch.cuda.synchronize()
    assert out.shape == (10,) and torch.isfinite(out).all() and int(out[6]) > 0 and int(out[9]) == int(out[6])
    assert all(torch.isfinite(b).all() for b in ts.grads.buckets) and torch.isfinite(ts.pj_grad).all()
    assert all(torch.isfinite(p).all() for p in hip.parameters())


def test_train_state_round_trips_mask_assign(tmp_path):
    xs, gt_boxes, gt_masks, gt_cls = _batch(13)
    kw = dict(optimizer="sgd", det_loss="tal", instance_mask_weight=1.0)
    a = TrainStep(build(6)[1], (B, 3, S, S), lr=0.05, mask_assign="tal", **kw)
    a.step(*_dev(xs[0], gt_boxes, gt_masks, gt_cls))
    path = tmp_path / "state.pt"
    save_train_state(path, a)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["mask_assign"] == "tal" and saved["det_loss"] == "tal" and saved["steps"] == 1
    b = TrainStep(build(7)[1], (B, 3, S, S), lr=0.01, mask_assign="tal", **kw)
    load_train_state(path, b)
    assert b.steps == 1 and b.lr == 0.05
    sa, sb = a.state_dict(), b.state_dict()
    assert sb["mask_assign"] == "tal" and all(torch.equal(sa["state_dict"][k], sb["state_dict"][k]) for k in sa["state_dict"])
    c = TrainStep(build(7)[1], (B, 3, S, S), lr=0.01, **kw)
    assert c.mask_assign == "iou" and c.state_dict()["mask_assign"] == "iou"
    with pytest.raises(ValueError, match="mask_assign"):
        load_train_state(path, c)
    legacy = {k: v for k, v in c.state_dict().items() if k != "mask_assign"}       # a state from before the key: the IoU match
    c.load_state_dict(legacy)
    with pytest.raises(ValueError, match="mask_assign"):
        b.load_state_dict(legacy)


def test_default_mask_assign_is_bit_identical_to_iou():
    xs, gt_boxes, gt_masks, gt_cls = _batch(13)
    outs, params = [], []
    for kw in ({}, {"mask_assign": "iou"}):
        _, hip = build(6)
        ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.05, iou_match_thresh=0.05, det_loss="tal", instance_mask_weight=1.0, **kw)
        assert ts.mask_assign == "iou"
        outs.append(ts.step(*_dev(xs[0], gt_boxes, gt_masks, gt_cls)).clone())
        torch.cuda.synchronize()
        params.append({n: p.detach().clone() for n, p in hip.named_parameters()})
    assert outs[0].shape == (10,) and torch.equal(outs[0], outs[1])
    assert int(outs[0][9]) > 0 and int(outs[0][6]) > 0                               # the IoU match at 0.05 has positives of its own
    assert all(torch.equal(params[0][n], params[1][n]) for n in params[0])
