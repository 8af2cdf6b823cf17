"""The assembled training step behind the Module (BASELINE configs[2]): `forward(x, "train")` under `model.train()` returns tensors
with autograd history; `.backward()` runs the HIP backward plan.  Every parameter gradient is compared with torch autograd through
the oracle model on the same state_dict and inputs (fp32 mode: <= 1e-3 relative to the gradient's largest entry).

Reference call stack this mirrors: `/root/reference/src/running_main_v3.py:393-445` (training_step -> _multitask_loss -> Lightning's
backward) over `/root/reference/src/main_model.py:342-365`."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, ConvNeXtBiFPNYOLOv2
    from oracle import loss as oloss
    from oracle.model import ConvNeXtBiFPNYOLO as OModel, ConvNeXtBiFPNYOLOv2 as OModelV2, randomize_


def build(variant="main", seed=0, train=True):
    torch.manual_seed(seed)
    ocls, hcls = (OModel, ConvNeXtBiFPNYOLO) if variant == "main" else (OModelV2, ConvNeXtBiFPNYOLOv2)
    ora = randomize_(ocls(2, 2, pretrained_backbone=False), seed)
    hip = hcls(2, 2, pretrained_backbone=False)
    hip.load_state_dict(ora.state_dict(), strict=True)
    hip = hip.to(DEV)
    ora.train(train)
    hip.train(train)
    return ora, hip


def flat_outputs(out):
    """(det list | absent, (seg list, mc, protos), logits) -> flat list of tensors in a fixed order"""
    if len(out) == 3:
        det, (seg, mc, protos), logits = out
        return list(det) + list(seg) + [mc, protos, logits]
    (seg, mc, protos), logits = out
    return list(seg) + [mc, protos, logits]


def compare_grads(ora, hip, rtol, what, allow_none=()):
    bad = []
    ref_scale = max(p.grad.abs().max().item() for p in ora.parameters() if p.grad is not None)
    hp = dict(hip.named_parameters())
    for name, p in ora.named_parameters():
        g = hp[name].grad
        if p.grad is None:
            assert g is None, f"{name}: oracle has no gradient, HIP has one"
            continue
        if g is None:
            if any(name.startswith(a) for a in allow_none):
                continue
            bad.append(f"{name}: missing")
            continue
        g = g.float().cpu()
        err = (g - p.grad).abs().max().item()
        scale = p.grad.abs().max().item()
        # absolute floor: conv biases in front of a batch-statistic BatchNorm have an exactly-zero gradient (autograd returns rounding
        # noise there), and a few scalars are tiny next to the rest of the network
        if err > rtol * scale + 1e-6 * ref_scale:
            bad.append(f"{name}: err {err:.3e} scale {scale:.3e} ({tuple(p.shape)})")
    assert not bad, f"{what}: {len(bad)} parameter gradients differ:\n" + "\n".join(bad[:60])


@pytest.mark.parametrize("variant", ["main", "v2"])
def test_every_parameter_gradient_matches_autograd_fp32(variant):
    """model.train(): batch-statistic BatchNorm everywhere (C2f slices included).  The loss is a fixed random linear functional of ALL
    outputs, so that every parameter -- Segment's cv2 / cv3 / cv4, which the reference's loss never reaches, included -- gets a gradient."""
    ora, hip = build(variant)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 128, 128, generator=g)
    ro = flat_outputs(ora(x, "train"))
    ho = flat_outputs(hip(x.to(DEV), "train"))
    worst = 0.0
    for r, h in zip(ro, ho):
        assert tuple(r.shape) == tuple(h.shape)
        worst = max(worst, (h.detach().float().cpu() - r.detach()).abs().max().item())
    assert worst < 1e-3, f"train-mode forward differs from the oracle by {worst}"
    probes = [torch.randn(r.shape, generator=g) / r[0].numel() ** 0.5 for r in ro]
    sum((r * w).sum() for r, w in zip(ro, probes)).backward()
    sum((h * w.to(DEV)).sum() for h, w in zip(ho, probes)).backward()
    torch.cuda.synchronize()
    compare_grads(ora, hip, 1e-3, f"{variant} fp32")
    # running statistics / num_batches_tracked moved exactly like the oracle's
    hb = dict(hip.named_buffers())
    for name, b in ora.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(hb[name]) == int(b), name
        elif name.endswith("running_mean") or name.endswith("running_var"):
            assert (hb[name].cpu() - b).abs().max().item() <= 1e-3 * (b.abs().max().item() + 1e-3), name


def test_src_model_py_variant_trains_fp32():
    """BASELINE config 0's graph (reference src/model.py:97-123) under module.train(): lateral Convs, the weight-ADDING WeightedAdd nodes over
    identity / nearest-x2 / max-pooled inputs, DWConv 3x3 + BatchNorm + SiLU, the heads' training outputs.  Forward and EVERY parameter
    gradient (the WeightedAdd weights included: one of them negative, relu' = 0) against autograd through the oracle."""
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLOv0
    from oracle.model import ConvNeXtBiFPNYOLOv0 as OModelV0
    torch.manual_seed(3)
    ora = randomize_(OModelV0(2, 2), 3)
    with torch.no_grad():
        for ui, u in enumerate(ora.neck.units):
            u.add_p4_td.w.copy_(torch.tensor([0.7, 1.3]) + 0.1 * ui)
            u.add_p3_td.w.copy_(torch.tensor([1.5, 0.4]))
            u.add_p4_out.w.copy_(torch.tensor([1.2, -0.3, 0.8]))
            u.add_p5_out.w.copy_(torch.tensor([0.9, 1.1]))
    hip = ConvNeXtBiFPNYOLOv0(2, 2)
    hip.load_state_dict(ora.state_dict(), strict=True)
    hip = hip.to(DEV)
    ora.train()
    hip.train()
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 128, 128, generator=g)
    ro = flat_outputs(ora(x, "train"))
    ho = flat_outputs(hip(x.to(DEV), "train"))
    worst = 0.0
    for r, h in zip(ro, ho):
        assert tuple(r.shape) == tuple(h.shape)
        worst = max(worst, (h.detach().float().cpu() - r.detach()).abs().max().item())
    assert worst < 1e-3, f"train-mode forward of the src/model.py variant differs from the oracle by {worst}"
    probes = [torch.randn(r.shape, generator=g) / r[0].numel() ** 0.5 for r in ro]
    sum((r * w).sum() for r, w in zip(ro, probes)).backward()
    sum((h * w.to(DEV)).sum() for h, w in zip(ho, probes)).backward()
    torch.cuda.synchronize()
    compare_grads(ora, hip, 1e-3, "src/model.py variant fp32")
    hb = dict(hip.named_buffers())
    for name, b in ora.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(hb[name]) == int(b), name
        elif name.endswith("running_mean") or name.endswith("running_var"):
            assert (hb[name].cpu() - b).abs().max().item() <= 1e-3 * (b.abs().max().item() + 1e-3), name
    # the dict form of the same call, and the mixed head modes the lowering refuses
    out = hip(x.to(DEV), "infer")
    assert isinstance(out["detect"], list) and len(out["detect"]) == 3 and len(out["segment"]) == 2 and out["img_cls"].shape == (2, 2)
    hip.detect.eval()
    with pytest.raises(NotImplementedError):
        hip(x.to(DEV), "train")
    # bf16 arithmetic: same plan shape, outputs within bf16 rounding of the fp32 oracle, a finite gradient for every parameter
    hip.train().set_compute_dtype(torch.bfloat16)
    hip.zero_grad(set_to_none=True)
    hb16 = flat_outputs(hip(x.to(DEV), "train"))
    for r, h in zip(ro, hb16):
        assert ((h.detach().float().cpu() - r.detach()).abs().max() / (r.detach().abs().max() + 1e-6)).item() < 8e-2
    sum((h * w.to(DEV)).sum() for h, w in zip(hb16, probes)).backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in hip.parameters() if p.requires_grad)


def test_training_step_with_the_reference_loss_fp32():
    """forward(train) -> the trainer's `_multitask_loss` (oracle restatement, plain torch ops on the returned tensors) -> backward:
    what `running_main_v3.py:393-445` does.  Only the Detect maps, the prototypes and the image logits reach the loss, so Segment's
    cv2 / cv3 / cv4 get NO gradient -- in the oracle and here alike."""
    ora, hip = build("main", seed=1)
    g = torch.Generator().manual_seed(7)
    S = 128
    x = torch.rand(2, 3, S, S, generator=g)
    gt_boxes = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 0, 0.4, 0.6, 0.5, 0.5]])
    gt_masks = torch.zeros(2, 1, S, S)
    gt_masks[0, 0, 45:83, 38:90] = 1
    gt_masks[1, 0, 45:109, 19:83] = 1
    gt_cls = torch.tensor([1, 0])
    proj = torch.nn.Conv2d(32, 1, 1)
    kw = dict(img_size=S, nc_det=2, iou_match_thresh=0.05, label_smoothing=0.1, training=True)     # low threshold: random heads still match

    det_r, (_, _, protos_r), logits_r = ora(x, "train")
    lr = oloss.multitask_loss(det_r, protos_r, logits_r, gt_boxes, gt_masks, gt_cls, proj.weight, proj.bias, **kw)
    # the same torch loss on CPU copies that keep the autograd link to the HIP outputs
    det, (seg, mc, protos), logits = hip(x.to(DEV), "train")
    lh = oloss.multitask_loss([d.cpu() for d in det], protos.cpu(), logits.cpu(), gt_boxes, gt_masks, gt_cls, proj.weight, proj.bias, **kw)
    assert lr[6].item() > 0, "the synthetic batch must produce positive matches"
    assert abs(lh[0].item() - lr[0].item()) <= 1e-3 * abs(lr[0].item())
    lr[0].backward()
    lh[0].backward()
    torch.cuda.synchronize()
    compare_grads(ora, hip, 1e-3, "reference loss fp32")
    hp = dict(hip.named_parameters())
    for name in ("segment.cv2.0.0.conv.weight", "segment.cv3.1.2.weight", "segment.cv4.2.2.bias"):
        assert hp[name].grad is None


def test_eval_mode_backbone_backward_fp32():
    """model.eval() with autograd on (frozen BatchNorm statistics in backbone / neck; the heads are flipped to train mode by forward,
    main_model.py:358-359): running-statistic BatchNorm backward, conv biases get real gradients."""
    ora, hip = build("main", seed=2, train=False)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 96, 96, generator=g)
    ro, ho = flat_outputs(ora(x, "train")), flat_outputs(hip(x.to(DEV), "train"))
    probes = [torch.randn(r.shape, generator=g) / r[0].numel() ** 0.5 for r in ro]
    sum((r * w).sum() for r, w in zip(ro, probes)).backward()
    sum((h * w.to(DEV)).sum() for h, w in zip(ho, probes)).backward()
    torch.cuda.synchronize()
    compare_grads(ora, hip, 1e-3, "eval-mode backbone fp32")


def test_bf16_training_step_gradients_are_close_and_finite():
    """bf16 storage (the throughput mode): gradients stay finite and point the same way as autograd's through the oracle.  The oracle
    runs in fp64: a conv bias in front of a batch-statistic BatchNorm has an exactly-zero gradient (HIP leaves it zero), and fp32
    autograd returns rounding noise there whose size -- above or below the 1e-6 floor -- depends on the host's CPU thread count."""
    ora, hip = build("main", seed=3)
    ora.double()
    hip.set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(4, 3, 128, 128, generator=g)
    ro, ho = flat_outputs(ora(x.double(), "train")), flat_outputs(hip(x.to(DEV), "train"))
    probes = [torch.randn(r.shape, generator=g) / r[0].numel() ** 0.5 for r in ro]
    sum((r * w.double()).sum() for r, w in zip(ro, probes)).backward()
    sum((h * w.to(DEV)).sum() for h, w in zip(ho, probes)).backward()
    torch.cuda.synchronize()
    hp = dict(hip.named_parameters())
    low = []
    for name, p in ora.named_parameters():
        if p.grad is None:                      # the frozen DFL projection
            assert hp[name].grad is None
            continue
        gh = hp[name].grad.float().cpu()
        assert torch.isfinite(gh).all(), name
        if p.grad.numel() < 64 or p.grad.abs().max().item() < 1e-6:
            continue
        cos = torch.nn.functional.cosine_similarity(gh.double().flatten(), p.grad.flatten(), dim=0).item()
        if cos < 0.9:
            low.append(f"{name}: cos {cos:.3f}")
    assert len(low) <= 8, "bf16 gradients diverge from fp64 autograd:\n" + "\n".join(low[:40])


def test_stale_backward_is_refused():
    ora, hip = build("main", seed=4)
    x = torch.rand(1, 3, 64, 64).to(DEV)
    out1 = hip(x, "train")
    hip(x, "train")                       # overwrites the kept activations of the first forward
    with pytest.raises(RuntimeError, match="overwritten"):
        out1[2].sum().backward()


def test_native_train_step_matches_torch_loop_fp32():
    """trainstep.TrainStep (forward -> device loss + gradient -> projector backward -> backward plan -> global-norm clip -> fused SGD over
    the re-homed flat buckets) against the same two steps done with torch on the oracle: autograd, clip_grad_norm_(10), torch.optim.SGD.
    Two steps, so that the second one runs on re-prepared weights, moved BatchNorm statistics and a live momentum buffer."""
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    ora, hip = build("main", seed=6)
    S, B = 128, 2
    g = torch.Generator().manual_seed(13)
    xs = [torch.rand(B, 3, S, S, generator=g) for _ in range(2)]
    gt_boxes = torch.tensor([[0, 1, 0.5, 0.5, 0.4, 0.3], [1, 0, 0.4, 0.6, 0.5, 0.5], [1, 1, 0.3, 0.3, 0.2, 0.25]])
    gt_masks = torch.zeros(B, 1, S, S)
    gt_masks[0, 0, 45:83, 38:90] = 1
    gt_masks[1, 0, 45:109, 19:83] = 1
    gt_cls = torch.tensor([1, 0])
    proj = torch.nn.Conv2d(32, 1, 1)
    proj_h = torch.nn.Conv2d(32, 1, 1)
    proj_h.load_state_dict(proj.state_dict())
    kw = dict(iou_match_thresh=0.05, label_smoothing=0.1)
    before = {n: p.detach().clone() for n, p in ora.named_parameters()}
    lr, wd, mom = 0.05, 5e-4, 0.9
    opt = torch.optim.SGD(list(ora.parameters()) + list(proj.parameters()), lr=lr, momentum=mom, weight_decay=wd)
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=lr, weight_decay=wd, momentum=mom, clip_norm=10.0, projector=proj_h, **kw)
    assert ts.n_skip >= 1
    for step, x in enumerate(xs):
        opt.zero_grad(set_to_none=True)
        det_r, (_, _, protos_r), logits_r = ora(x, "train")
        lr_ = oloss.multitask_loss(det_r, protos_r, logits_r, gt_boxes, gt_masks, gt_cls, proj.weight, proj.bias, img_size=S, nc_det=2, training=True, **kw)
        lr_[0].backward()
        total = torch.nn.utils.clip_grad_norm_(list(ora.parameters()) + list(proj.parameters()), 10.0)
        opt.step()
        lh = ts.step(x.to(DEV), gt_boxes.to(DEV), gt_masks.to(DEV), gt_cls.to(DEV))
        torch.cuda.synchronize()
        assert abs(lh[0].item() - lr_[0].item()) <= 2e-3 * abs(lr_[0].item()), (step, lh[0].item(), lr_[0].item())
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
    assert (proj_h.weight.detach().cpu() - proj.weight.detach()).abs().max().item() <= 2e-3 * (proj.weight.detach() - 0).abs().max().item()
    # Segment's cv2 / cv3 / cv4 never reach the loss: untouched, like torch's optimisers leave parameters without a gradient
    assert torch.equal(hp["segment.cv4.0.0.conv.weight"].detach().cpu(), before["segment.cv4.0.0.conv.weight"])


def test_two_rank_step_equals_averaged_gradients(tmp_path):
    """BASELINE configs[3] in miniature: two ranks (one process each, `gloo` rehearsal backend on the shared GPU; "nccl" = RCCL on a real node)
    run `TrainStep.step` on the two halves of a batch with the bucketed all-reduce overlapped with backward.  The parameters they end with must
    equal those of ONE process that computes the two shards' gradients separately, averages them and applies the same clip + SGD update --
    twice, so that the second step starts from exchanged weights."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import ddp_worker as W
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    out = str(tmp_path / "ddp.pt")
    env = dict(os.environ, MTBT_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29533", os.path.join(root, "tools", "ddp_worker.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = torch.load(out, weights_only=True)
    assert got["side_stream_all_reduce"] is True or str(got["side_stream_all_reduce"]).startswith("skipped"), got["side_stream_all_reduce"]
    # ---- the same two steps in one process: per-shard gradients, averaged by hand ----
    S, per = 128, 2
    model = W.build_model(torch.device(DEV))
    torch.manual_seed(3)
    proj = torch.nn.Conv2d(32, 1, 1)
    ts = TrainStep(model, (per, 3, S, S), projector=proj, **W.STEP_KW)
    batch = W.make_batch(S, 2 * per)
    for step in range(2):
        acc, accp = None, None
        for rank in range(2):
            x, bx, mk, cl = (t.to(DEV) for t in W.shard(batch, rank, per))
            ts.forward_backward(x, bx, mk, cl)
            gs = [b.clone() for b in ts.grads.buckets]
            acc = gs if acc is None else [a + b for a, b in zip(acc, gs)]
            accp = ts.pj_grad.clone() if accp is None else accp + ts.pj_grad
        for b, a in zip(ts.grads.buckets, acc):
            b.copy_(a / 2)
        ts.pj_grad.copy_(accp / 2)
        ts._clip_and_update()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got["buckets"], ts.params.buckets)):
        err = (a - b.cpu()).abs().max().item()
        assert err <= 1e-5 * (b.abs().max().item() + 1e-6) + 1e-7, f"parameter bucket {i}: {err}"
    assert (got["proj"] - ts.pj.cpu()).abs().max().item() <= 1e-5


def test_training_plans_on_lanes_are_bit_identical(monkeypatch):
    """MTBT_TRAIN_LANES=1 spreads the forward / backward launches over the engine's HIP streams following the recorded read / write regions
    (per-launch scratch buffers, parameter-gradient slots tracked by element range).  No atomics anywhere, so every gradient must equal
    the single-stream result BIT FOR BIT -- a missing dependency shows up here as a difference."""
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    ora, hip = build("main", seed=12)
    hip.set_compute_dtype(torch.bfloat16)
    S, B = 256, 4
    g = torch.Generator().manual_seed(17)
    x = torch.rand(B, 3, S, S, generator=g).to(DEV)
    gt_boxes = torch.tensor([[b, b % 2, 0.4 + 0.05 * b, 0.5, 0.3, 0.35] for b in range(B)], dtype=torch.float32).to(DEV)
    gt_masks = torch.zeros(B, 1, S, S, device=DEV)
    gt_masks[:, 0, 60:140, 50:170] = 1
    gt_cls = torch.tensor([0, 1, 1, 0]).to(DEV)
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=0.0, iou_match_thresh=0.05)     # lr 0: the weights stay put between the runs
    # the BatchNorm running statistics are part of the state a step reads (the conv epilogue accumulates its column sums about the running
    # mean): every run starts from the same copy
    bufs = {n: b.clone() for n, b in hip.named_buffers()}

    def reset():
        with torch.no_grad():
            for n, b in hip.named_buffers():
                b.copy_(bufs[n])
    monkeypatch.setenv("MTBT_TRAIN_LANES", "0")
    ts.tp.reload_env()                                   # (the lane knobs are read once per plan)
    ts.forward_backward(x, gt_boxes, gt_masks, gt_cls)
    torch.cuda.synchronize()
    ref = [b.clone() for b in ts.grads.buckets]
    monkeypatch.setenv("MTBT_TRAIN_LANES", "1")
    monkeypatch.setenv("MTBT_LANES", "4")
    ts.tp.reload_env()
    for _ in range(6):
        reset()
        ts.forward_backward(x, gt_boxes, gt_masks, gt_cls)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(ref, ts.grads.buckets)):
            assert torch.equal(a, b), f"gradient bucket {i} differs between single-stream and lane execution"


def test_gradient_accumulation_over_two_backward_passes_fp32():
    """Two forward + backward passes WITHOUT zero_grad (gradient accumulation, `zero_grad(set_to_none=False)`): `.grad` = g1 + g2 as with
    autograd through the oracle.  The autograd node hands out views of fresh per-backward copies of the gradient buckets; round 2 handed
    out views of the persistent arena, which AccumulateGrad keeps as `.grad` without a copy where the strides match (stem weight, 1x1
    depthwise weights, class bias): the second pass then rewrote `.grad` in place and added the buffer to itself (2*g2)."""
    ora, hip = build("main", seed=3)
    g = torch.Generator().manual_seed(23)
    xs = [torch.rand(2, 3, 64, 64, generator=g) for _ in range(2)]
    first = {}
    for k, x in enumerate(xs):
        ro = flat_outputs(ora(x, "train"))
        ho = flat_outputs(hip(x.to(DEV), "train"))
        probes = [torch.randn(r.shape, generator=g) / r[0].numel() ** 0.5 for r in ro]
        sum((r * w).sum() for r, w in zip(ro, probes)).backward()
        sum((h * w.to(DEV)).sum() for h, w in zip(ho, probes)).backward()
        torch.cuda.synchronize()
        if k == 0:
            first = {n: (p.grad, p.grad.clone()) for n, p in hip.named_parameters() if p.grad is not None}
    compare_grads(ora, hip, 1e-3, "accumulated over two passes")
    # a `.grad` tensor saved after the first pass is never a window onto memory the second pass rewrites: autograd accumulated into it
    # (in place), so it now holds g1 + g2 and differs from its own first-pass value by exactly the oracle's second-pass gradient
    tp = next(iter(hip._train_plans.values()))
    arena = {b.untyped_storage().data_ptr() for b in tp.arena.buckets}
    for n, p in hip.named_parameters():
        if p.grad is not None:
            assert p.grad.untyped_storage().data_ptr() not in arena, f"{n}.grad aliases the persistent gradient arena"
    for n in ("backbone.body.stem_0.weight", "neck.bifpn_units.0.p4_td_conv.depthwise.weight", "detect.cv3.0.2.bias"):
        kept, old = first[n]
        assert kept is dict(hip.named_parameters())[n].grad and not torch.equal(kept, old)


def test_backward_plan_does_not_depend_on_an_earlier_backward_plan_fp32():
    """A backward plan lowered after another one (here: for `logits` alone) is the plan a fresh model lowers first: two identically
    seeded models run the same two train-mode forwards (so the BatchNorm running means that shift the fused column sums agree); A also
    back-propagates a loss on the logits after its first forward and zeroes its gradients, both back-propagate the same loss on every
    output after the second.  Same plans, no atomics: every parameter gradient agrees bit for bit."""
    g = torch.Generator().manual_seed(31)
    xs = [torch.rand(2, 3, 64, 64, generator=g).to(DEV) for _ in range(2)]
    probes = None
    grads = []
    for with_first_backward in (True, False):
        _, hip = build("main", seed=5)
        out = hip(xs[0], "train")
        if with_first_backward:
            out[2].square().sum().backward()
            hip.zero_grad(set_to_none=True)
        ho = flat_outputs(hip(xs[1], "train"))
        if probes is None:
            probes = [(torch.randn(h.shape, generator=g) / h[0].numel() ** 0.5).to(DEV) for h in ho]
        sum((h * w).sum() for h, w in zip(ho, probes)).backward()
        torch.cuda.synchronize()
        grads.append({n: p.grad for n, p in hip.named_parameters()})
        tp, = hip._train_plans.values()
        assert len(tp._bwd_cache) == (2 if with_first_backward else 1)
    a, b = grads
    assert any(v is not None for v in b.values())
    for n in a:
        assert (a[n] is None) == (b[n] is None), n
        assert a[n] is None or torch.equal(a[n], b[n]), f"{n}: gradient depends on the backward plan lowered before"


def test_bf16_fused_mlp_lowering_agrees_with_the_two_gemm_lowering(monkeypatch):
    """bf16 training plan: stages 0-1 run the ConvNeXt Mlp as one launch that keeps only the fc1 pre-activation (mtbt_convnext_mlp_fused_train,
    the fc2 weight gradient re-applies GELU while staging it).  Against the same plan built with MTBT_TRAIN_FUSED_MLP=0 (fc1 / fc2 as two GEMMs, the
    activated tensor kept): outputs and the block's parameter gradients agree to bf16 accuracy."""
    import importlib
    from multitask_bonetumor_yolo_amd import train as T
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(T, "FUSED_TRAIN_MLP", fused)
        _, hip = build("main", seed=6, train=False)      # BatchNorm on running statistics: no batch-of-2 statistics to amplify rounding differences
        hip.set_compute_dtype(torch.bfloat16)
        det, (seg, mc, protos), logits = hip(x, "train")
        names = [l.name for l in next(iter(hip._train_plans.values())).fwd.launches]
        assert any("mlp(fused)" in n for n in names) == fused
        (sum(d.float().mean() for d in det) + protos.float().mean() + logits.float().sum()).backward()
        torch.cuda.synchronize()
        gr = {n: p.grad.float().clone() for n, p in hip.named_parameters() if p.grad is not None and ("stages_0.blocks.0" in n or "stages_1.blocks.2" in n)}
        res[fused] = ([d.float().clone() for d in det] + [protos.float().clone(), logits.float().clone()], gr)
    for a, b in zip(res[True][0], res[False][0]):
        assert (a - b).norm().item() <= 3e-2 * b.norm().item() + 1e-3
    assert res[True][1].keys() == res[False][1].keys() and len(res[True][1]) >= 10
    for n, gb in res[False][1].items():
        ga = res[True][1][n]
        cos = torch.nn.functional.cosine_similarity(ga.flatten(), gb.flatten(), dim=0).item()
        assert cos >= 0.97 or gb.norm().item() < 1e-6, (n, cos)


def test_forward_follows_the_trainers_autocast():
    """`precision="bf16-mixed"` (running_main_v3.py:825): Lightning wraps forward in autocast("cuda", bfloat16).  A drop-in whose arithmetic
    mode was never pinned follows it -- the bf16 training / inference plans are the ones lowered and run, the outputs stay fp32 tensors, the
    backward works outside the autocast region (as Lightning calls it) -- and a pinned mode is not overridden."""
    ora, hip = build("main", seed=4)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(31)).to(DEV)
    assert hip.compute_dtype == torch.float32
    with torch.autocast("cuda", torch.bfloat16):
        assert hip.compute_dtype == torch.bfloat16
        det, (seg, mc, protos), logits = hip(x, "train")
        loss = sum(d.float().mean() for d in det) + protos.float().mean() + logits.float().sum()
    assert all(t.dtype == torch.float32 for t in list(det) + [mc, protos, logits])
    loss.backward()
    torch.cuda.synchronize()
    assert [k[1] for k in hip._train_plans] == [torch.bfloat16]
    g16 = {n: p.grad.float().clone() for n, p in hip.named_parameters() if p.grad is not None}
    assert g16 and all(torch.isfinite(g).all() for g in g16.values())
    hip.zero_grad(set_to_none=True)
    det, (seg, mc, protos), logits = hip(x, "train")                      # outside autocast: the fp32 parity mode, a second plan
    (sum(d.mean() for d in det) + protos.mean() + logits.sum()).backward()
    torch.cuda.synchronize()
    assert sorted(str(k[1]) for k in hip._train_plans) == ["torch.bfloat16", "torch.float32"]
    # the same gradient in bf16 arithmetic.  Checked where it is a property of the arithmetic: cls_fc's weight gradient is the pooled P5
    # feature (d logits.sum()).  Deep inside a random-initialised net with batch-statistics BN over 2 x 2 x 2 positions the backward is
    # chaotic (round 3: 80 % relative difference on a P3 weight at this size) and says nothing about the mode.
    name = "cls_fc.weight"
    g32 = dict(hip.named_parameters())[name].grad.float()
    cos = torch.nn.functional.cosine_similarity(g16[name].flatten(), g32.flatten(), dim=0).item()
    assert cos >= 0.9, cos
    hip.eval()
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        out = hip(x, "infer")
    assert out["img_cls_logits"].dtype == torch.float32 and any(k[1] == torch.bfloat16 for k in hip._plans)
    hip.set_compute_dtype(torch.float32)
    with torch.no_grad(), torch.autocast("cuda", torch.bfloat16):
        assert hip.compute_dtype == torch.float32                          # pinned: autocast is not consulted
    with torch.autocast("cuda", torch.float16):
        hip.set_compute_dtype(None).train()
        with pytest.raises(NotImplementedError):
            hip(x, "train")                                                # fp16 is an inference mode


def test_two_rank_overlapped_exchange_is_bit_identical_to_sequential(tmp_path):
    """configs[3]'s exchange at a size where the backward plan really spreads over its four lanes (2 ranks x 4 x 256^2, bf16, MTBT_TRAIN_LANES=1):
    with the bucket all-reduces OVERLAPPED with backward (side stream, one event per writer lane) the parameters after two steps are
    bit-identical to the run that reduces after the whole backward pass.  A collective that started before one of its bucket's writers had
    finished (round 2's single-event wait) shows up here as a difference."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for overlap in ("1", "0"):
        out = str(tmp_path / f"ddp_{overlap}.pt")
        env = dict(os.environ, MTBT_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", MTBT_DDP_OVERLAP=overlap,
                   MTBT_DDP_S="256", MTBT_DDP_PER="4", MTBT_DDP_DTYPE="bf16", MTBT_TRAIN_LANES="1", MTBT_LANES="4")
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                            "--master-port", "29537", os.path.join(root, "tools", "ddp_worker.py"), out], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs[overlap] = torch.load(out, weights_only=True)
    a, b = outs["1"], outs["0"]
    assert all(torch.isfinite(t).all() for t in a["buckets"])
    for i, (u, v) in enumerate(zip(a["buckets"], b["buckets"])):
        assert torch.equal(u, v), f"parameter bucket {i}: overlapped exchange != sequential exchange (max diff {(u - v).abs().max().item():.3e})"
    assert torch.equal(a["proj"], b["proj"]) and all(torch.equal(x, y) for x, y in zip(a["losses"], b["losses"]))


def test_train_step_at_configs2_size_bf16(monkeypatch):
    """BASELINE configs[2] at its real size -- ONE `TrainStep.step` of batch 32 x 640^2 in bf16 (SGD, clip 10): the 20.8 GiB activation arena,
    the 1024-workgroup weight-gradient splits and the batch-32 tile choices, through size-independent properties: finite loss and gradient
    norm, positives found, every reduced gradient bucket finite and non-zero, and the gradients of the 4-lane execution bit-identical
    to single-stream execution of the same plans."""
    import os
    import sys
    from multitask_bonetumor_yolo_amd import init_synthetic_
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import synthetic_targets
    torch.manual_seed(0)
    B, S = 32, 640
    hip = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(DEV).set_compute_dtype(torch.bfloat16)
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(DEV)
    boxes, masks, cls = synthetic_targets(B, S, 0, torch.device(DEV))
    monkeypatch.setenv("MTBT_TRAIN_LANES", "1")
    monkeypatch.setenv("MTBT_LANES", "4")
    ts = TrainStep(hip, (B, 3, S, S), optimizer="sgd", lr=1e-4, iou_match_thresh=0.05)
    assert ts.tp.fwd.pool.bytes > 15 * 2 ** 30                                  # the kept activations of the real configuration
    bufs = {n: b.clone() for n, b in hip.named_buffers()}
    ts.forward_backward(x, boxes, masks, cls)
    torch.cuda.synchronize()
    lanes = [b.clone() for b in ts.grads.buckets]
    with torch.no_grad():
        for n, b in hip.named_buffers():
            b.copy_(bufs[n])                                                     # (the column sums are taken about the running mean)
    monkeypatch.setenv("MTBT_TRAIN_LANES", "0")
    ts.tp.reload_env()
    ts.forward_backward(x, boxes, masks, cls)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(lanes, ts.grads.buckets)):
        assert torch.equal(a, b), f"gradient bucket {i}: lanes != single stream at batch 32 x 640^2"
    monkeypatch.setenv("MTBT_TRAIN_LANES", "1")
    ts.tp.reload_env()
    before = [b.clone() for b in ts.params.buckets]
    loss = ts.step(x, boxes, masks, cls)
    torch.cuda.synchronize()
    lv = loss.float().cpu()
    assert torch.isfinite(lv).all() and lv[6].item() > 0, lv                     # total ... #positives > 0
    assert torch.isfinite(ts.gnorm).all() and ts.gnorm.item() > 0
    for i in range(ts.n_skip, len(ts.grads.buckets)):
        g = ts.grads.buckets[i]
        assert torch.isfinite(g).all() and g.abs().max().item() > 0, f"gradient bucket {i}"
        assert not torch.equal(before[i], ts.params.buckets[i]), f"parameter bucket {i} did not move"
    for i in range(ts.n_skip):
        assert torch.equal(before[i], ts.params.buckets[i])                      # Segment cv2 / cv3 / cv4: never stepped
