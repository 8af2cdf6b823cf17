"""The whole training step of BASELINE configs[2]-[3] as device work with no autograd graph and no host synchronisation:

    forward (train.TrainPlan) -> `_multitask_loss` + its gradient (csrc/loss.hip) -> proto-projector backward -> backward plan
    -> [data-parallel: one RCCL all-reduce per gradient bucket, issued on a side stream the moment the bucket's last producer has
       been launched, so that it runs UNDER the rest of the backward pass] -> global-norm clip -> fused AdamW / SGD over flat buckets

It is what `/root/reference/src/running_main_v3.py:393-445` (`training_step`) + Lightning's `backward` / `clip_gradients(10)` /
`optimizer.step()` (`:732-743`, `:824-828`) do per batch, with the reference's hyper-parameters as defaults.  The drop-in route --
`model(x, "train")` returning autograd tensors for the reference's own Lightning loop -- is `train.train_forward`; this class is the
same two launch plans driven natively.

Parameters are RE-HOMED once into flat fp32 buckets (`dist_train.FlatBuckets`) laid out exactly like the gradient buckets -- each
`nn.Parameter` keeps its name, shape and values but becomes a (channels-last) view of a bucket -- so the optimiser is one fused
launch per bucket and DDP's "unused parameter" problem (Segment.cv2 / cv3 / cv4 never reach the loss) is solved by
layout: those parameters live in their own leading bucket that is neither reduced nor stepped, which is also what torch's
optimisers do with `grad is None`.

`ema=` keeps an exponential moving average of every parameter and floating-point buffer (ultralytics' `ModelEMA`; the reference trainer
has none) in a second set of buckets of the same layout, updated by the optimiser launches themselves (`mtbt_*_step_ema`), and exposes
it as `ema_model` / `ema_projector`.  `state_dict()` / `load_state_dict()` carry everything a step needs to continue where it stopped.
"""
import copy
import math
from typing import Optional, Sequence

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L
from .engine import code_of, reserved_stream
from .loss import instance_mask_loss, multitask_loss, seg_region_loss, task_aligned_det_loss
from .dist_train import FlatBuckets
from .train import TrainPlan, make_arena

UNUSED_BY_THE_LOSS = ("segment.cv2.", "segment.cv3.", "segment.cv4.")   # running_main_v3.py:239-257 reads only seg_head_outputs[2]
UNUSED_WITH_MASK_LOSS = ("segment.cv2.", "segment.cv3.")                 # the instance-mask term reaches the coefficient branch (cv4)


EMA_DEFAULTS = dict(decay=0.9999, tau=2000.0)
PROJECTOR_KEYS = ("seg_proto_projector.weight", "seg_proto_projector.bias")    # the trainer's own entries of a Lightning checkpoint


def ema_decay_at(u: int, decay: float, tau: Optional[float]) -> float:
    """Decay of EMA update `u` (counted from 1): `decay * (1 - exp(-u / tau))`, `ModelEMA`'s ramp -- early updates follow the weights
    closely, later ones tend to `decay`.  `tau` 0 or None: constant `decay`.  Python floats."""
    if not tau:
        return float(decay)
    return float(decay) * (1.0 - math.exp(-u / tau))


def _ema_config(ema):
    """None | True | dict(decay=, tau=) -> None | (decay, tau)"""
    if ema is None or ema is False:
        return None
    cfg = dict(EMA_DEFAULTS)
    if ema is not True:
        unknown = set(ema) - set(cfg)
        if unknown:
            raise ValueError(f"ema: unknown keys {sorted(unknown)} (expected decay, tau)")
        cfg.update(ema)
    decay, tau = float(cfg["decay"]), cfg["tau"]
    if not 0.0 <= decay <= 1.0:
        raise ValueError("ema: decay must lie in [0, 1]")
    if tau is not None and float(tau) < 0:
        raise ValueError("ema: tau must be >= 0 (0 or None: constant decay)")
    return decay, (float(tau) if tau else None)


def _cpu(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", copy=True).contiguous()


def bucket_writers(launches, buckets):
    """Per flat bucket the indices of ALL launches that write into its storage, found from the write REGIONS the op builders record
    (`engine._region`: storage address + element range), not from tensor identity -- a derived view of a slot (`.view(-1)`) counts."""
    key = {b.untyped_storage().data_ptr(): k for k, b in enumerate(buckets)}
    out = [[] for _ in buckets]
    for i, l in enumerate(launches):
        for k in sorted({key[w[0]] for w in l.writes if w[0] in key}):
            out[k].append(i)
    return out


def exchange_marks(writers, live):
    """(marks for Plan.run, the order in which the collectives are issued): every writer of every live bucket is marked; buckets are
    reduced in the order of their latest writer; a bucket without a recorded writer comes last (it waits for the whole plan)."""
    marks = {str(b): list(writers[b]) for b in live if writers[b]}
    order = sorted(live, key=lambda k: (max(writers[k]) if writers[k] else 1 << 60, k))
    return marks, order


class TrainStep:
    def __init__(self, model, batch_shape: Sequence[int], *, optimizer: str = "adamw", lr: float = 1e-4, weight_decay: float = 5e-4,
                 betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.9, nesterov: bool = False, clip_norm: Optional[float] = 10.0,
                 iou_match_thresh: float = 0.5, label_smoothing: float = 0.1, loss_weights=(1.0, 2.0, 1.5, 0.5, 1.0),
                 projector: Optional[nn.Conv2d] = None, process_group=None, overlap: bool = True, instance_mask_weight: float = 0.0, ema=None,
                 det_loss: str = "reference", tal=None, mask_assign: str = "iou", seg_dice_weight: float = 0.0,
                 seg_boundary_weight: float = 0.0, seg_dice_smooth: float = 1.0):
        """batch_shape [B,3,S,S] per rank.  `projector` = the trainer's `seg_proto_projector` (Conv2d(proto_ch, 1, 1),
        running_main_v3.py:186); created (seeded default init) when not given.  A live `torch.distributed` process group with more than
        one rank turns on the gradient exchange; parameters are broadcast from rank 0 first (what DDP does at construction).
        `instance_mask_weight` > 0 adds `weight * instance_mask_loss` (csrc/mask_loss.hip; not a term of the reference's loss) to the
        total: Segment.cv4 then trains like any other parameter and the step returns 10 elements.  At 0 (default) nothing changes.
        `ema` = dict(decay=0.9999, tau=2000.0) (or True for those values) keeps averaged weights: `self.ema` (buckets laid out like
        `self.params`), `self.pj_ema`, `self.ema_model` / `self.ema_projector` (eval-mode modules over that storage, for validation
        and export); update u uses `ema_decay_at(u, decay, tau)`.  The model's floating-point buffers are then re-homed into one flat
        buffer so that one launch averages them all.  None (default): no launch, no storage and no buffer moves.
        `det_loss="tal"` replaces the detection terms of the reference's loss by the task-aligned detection loss (csrc/det_loss_tal.hip,
        `tal` = dict(topk=10, alpha=0.5, beta=6.0)): box / dfl / cls_det, #positives and the mean matched IoU of the returned tuple then
        hold its terms, its #foreground anchors and their mean overlap, weighted by the same `loss_weights` slots; `iou_match_thresh` then
        governs only the instance-mask term.  "reference" (default): nothing changes.
        `mask_assign="tal"` (needs `det_loss="tal"` and `instance_mask_weight` > 0) gives the instance-mask term the task-aligned
        assignment's foreground anchors and their assigned GT rows in place of its own IoU match (`v8SegmentationLoss`): the mask
        positives' count (element 9) then equals the number of foreground anchors (element 6) and `iou_match_thresh` is not read.
        "iou" (default): nothing changes.
        `seg_dice_weight` / `seg_boundary_weight` > 0 add the region terms of `loss.seg_region_loss` (csrc/distance_transform.hip: soft
        Dice with `seg_dice_smooth`, Kervadec's boundary loss over the device distance transform of the step's masks; not terms of the
        reference's loss) to the total: their gradient is added to the BCE gradient of the segmentation logits before the projector's
        backward, and two elements are appended after everything else: dice, boundary.  They are plain attributes of the same names,
        read at every step, so a schedule is an assignment between steps.  With both at 0 (default) nothing changes."""
        self.seg_dice_weight, self.seg_boundary_weight, self.seg_dice_smooth = float(seg_dice_weight), float(seg_boundary_weight), float(seg_dice_smooth)
        if not self.seg_dice_weight >= 0 or not self.seg_boundary_weight >= 0 or not self.seg_dice_smooth >= 0:
            raise ValueError("seg_dice_weight, seg_boundary_weight and seg_dice_smooth must be >= 0")
        if det_loss not in ("reference", "tal"):
            raise ValueError(f"det_loss: 'reference' (the reference trainer's _multitask_loss) or 'tal' (task-aligned), not {det_loss!r}")
        self.det_loss = det_loss
        self.tal_kw = dict(topk=10, alpha=0.5, beta=6.0)
        if tal is not None:
            if det_loss != "tal" or set(tal) - set(self.tal_kw):
                raise ValueError("tal: dict(topk=, alpha=, beta=), only with det_loss='tal'")
            self.tal_kw.update(tal)
        if mask_assign not in ("iou", "tal"):
            raise ValueError(f"mask_assign: 'iou' (the mask loss's own IoU match) or 'tal' (the task-aligned assignment), not {mask_assign!r}")
        if mask_assign == "tal" and (det_loss != "tal" or not float(instance_mask_weight) > 0):
            raise ValueError("mask_assign='tal' needs det_loss='tal' and instance_mask_weight > 0")
        self.mask_assign = mask_assign
        if not hasattr(model, "detect"):
            raise NotImplementedError("TrainStep drives the canonical model (running_main_v3.py needs .detect, SURVEY F4)")
        self.m = model
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("TrainStep: the model must live on an MI355X (no CPU path)")
        self.dev, self.lib = dev, L.load()
        self.B, _, self.S, _ = batch_shape
        model.train()
        self.projector = projector if projector is not None else nn.Conv2d(model.proto_ch, 1, 1)
        self.projector.to(dev)
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.group = process_group
        self._host_staged = self._host_staged_logged = False
        # ---- re-home the parameters into flat buckets with the gradient arena's layout ----
        self.mask_w = float(instance_mask_weight)
        if self.mask_w < 0:
            raise ValueError("instance_mask_weight must be >= 0")
        unused = UNUSED_WITH_MASK_LOSS if self.mask_w > 0 else UNUSED_BY_THE_LOSS
        self.params, gview, self.n_skip = make_arena(model, dev, unused)
        self._gview = gview
        self.ema_cfg = _ema_config(ema)
        self.ema = self.bufs = None
        self.ema_updates = 0
        with torch.no_grad():
            for name, p in model.named_parameters():
                if not p.requires_grad:
                    continue
                v = gview[name](self.params.views[name])
                v.copy_(p.data)
                p.data = v
            if self.ema_cfg is not None:                   # before the TrainPlan: it takes the buffers' pointers when it is built
                self.bufs, self.nbt = self._rehome_buffers(model)
            if self.world > 1:
                for t in list(self.params.buckets) + list(model.buffers()) + [p.data for p in self.projector.parameters()]:
                    self._bcast(t, 0)
        model.__dict__.pop("_train_plans", None)
        self.tp = TrainPlan(model, tuple(batch_shape), dev, code_of(model.compute_dtype), tail_prefixes=unused)
        assert [b.numel() for b in self.tp.arena.buckets] == [b.numel() for b in self.params.buckets]
        self.grads = self.tp.arena
        self.active = ("det", "logits", "protos") + (("mc",) if self.mask_w > 0 else ())
        self.bwd = self.tp.backward_plan(self.active)
        # the projector's three tensors: tiny flat buffers of their own
        nm = model.proto_ch
        self.pj = torch.zeros(nm + 4, device=dev)                      # weight [nm], bias [1]
        self.pj_grad, self.pj_m, self.pj_v = torch.zeros_like(self.pj), torch.zeros_like(self.pj), torch.zeros_like(self.pj)
        with torch.no_grad():
            self.pj[:nm].copy_(self.projector.weight.detach().view(-1))
            self.pj[nm:nm + 1].copy_(self.projector.bias.detach().view(-1))
            self.projector.weight.data = self.pj[:nm].view(1, nm, 1, 1)
            self.projector.bias.data = self.pj[nm:nm + 1]
        nb = self.lib.mtbt_projector_backward_workspace_bytes(self.B, self.S // 4, self.S // 4, nm)
        self.pj_ws = torch.empty(nb // 4, device=dev)
        # ---- optimiser state over the stepped buckets ----
        self.opt, self.lr, self.wd, self.betas, self.eps = optimizer, lr, weight_decay, betas, eps
        self.momentum, self.nesterov, self.clip_norm = momentum, nesterov, clip_norm
        if optimizer not in ("adamw", "sgd"):
            raise ValueError("optimizer: 'adamw' (the reference trainer, running_main_v3.py:732) or 'sgd' (BASELINE configs[2])")
        self.m1 = [torch.zeros_like(b) for b in self.params.buckets]
        self.m2 = [torch.zeros_like(b) for b in self.params.buckets] if optimizer == "adamw" else None
        self.steps = 0
        if self.ema_cfg is not None:
            self._make_ema(unused)
        self.sq, self.coef, self.gnorm = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.zeros(1, device=dev)
        self.sq_ws = torch.empty(self.lib.mtbt_sumsq_workspace_bytes() // 4, device=dev)
        self.loss_kw = dict(img_size=self.S, nc_det=model.nc_det, reg_max=model.detect.reg_max, iou_match_thresh=iou_match_thresh,
                            label_smoothing=label_smoothing, training=True, weights=loss_weights)
        if det_loss == "tal":        # the detection terms come from the task-aligned operator: the reference's get weight 0
            w = tuple(float(v) for v in loss_weights)
            self.tal_w = w[1:4]
            self.loss_kw["weights"] = (w[0], 0.0, 0.0, 0.0, w[4])
        # ---- gradient exchange: bucket b is complete once EVERY backward launch in writers[b] has run ----
        self.comm = reserved_stream(dev, "grad_exchange") if (self.world > 1 and overlap) else None
        self.writers = bucket_writers(self.bwd.launches, self.grads.buckets)

    # ------------------------------------------------------------------------------------------------------------------
    def _rehome_buffers(self, model):
        """Every floating-point buffer (BatchNorm running mean / var) becomes a view of ONE flat fp32 buffer, every integer one
        (`num_batches_tracked`) a view of one flat int64 tensor: the EMA of all of them is then one launch and one copy per step."""
        floats = [(n, b) for n, b in model.named_buffers() if b.is_floating_point()]
        for n, b in floats:
            if b.dtype != torch.float32:
                raise NotImplementedError(f"TrainStep(ema=...): buffer {n} is {b.dtype}, expected float32")
        self._buf_specs = [(n, tuple(b.shape)) for n, b in floats]
        flat = FlatBuckets(self._buf_specs, self.dev, bucket_bytes=1 << 62)
        assert len(flat.buckets) <= 1
        for n, b in floats:
            flat.views[n].copy_(b)
            b.data = flat.views[n]
        ints = [(n, b) for n, b in model.named_buffers() if not b.is_floating_point()]
        nbt = torch.zeros(len(ints), dtype=torch.int64, device=self.dev)
        for i, (n, b) in enumerate(ints):
            if b.dtype != torch.int64 or b.numel() != 1:
                raise NotImplementedError(f"TrainStep(ema=...): buffer {n} ({b.dtype}, {tuple(b.shape)}) is neither float nor a counter")
            nbt[i:i + 1].view(b.shape).copy_(b)
            b.data = nbt[i:i + 1].view(b.shape)
        return flat, nbt

    @torch.no_grad()
    def _make_ema(self, unused):
        """EMA storage = twins of the parameter arena, the buffer storage and the projector's flat buffer, starting as copies; the EMA
        model / projector are eval-mode copies of the live modules whose tensors are views of that storage."""
        model, dev, nm = self.m, self.dev, self.m.proto_ch
        self.ema, gview, n_skip = make_arena(model, dev, unused)          # the same model: the same layout by construction
        assert n_skip == self.n_skip and self.ema.layout == self.params.layout
        for e, p in zip(self.ema.buckets, self.params.buckets):
            e.copy_(p)
        self.ema_bufs = FlatBuckets(self._buf_specs, dev, bucket_bytes=1 << 62)
        assert self.ema_bufs.layout == self.bufs.layout
        for e, b in zip(self.ema_bufs.buckets, self.bufs.buckets):
            e.copy_(b)
        self.ema_nbt = self.nbt.clone()
        self.pj_ema = self.pj.clone()
        plans = {k: model.__dict__.pop(k) for k in ("_plans", "_train_plans") if k in model.__dict__}     # lowered plans are not copied
        try:
            self.ema_model = copy.deepcopy(model)
        finally:
            model.__dict__.update(plans)
        self.ema_model.requires_grad_(False).eval()
        live = dict(model.named_parameters())
        for name, p in self.ema_model.named_parameters():
            if name in gview and live[name].requires_grad:
                p.data = gview[name](self.ema.views[name])
        i = 0
        for name, b in self.ema_model.named_buffers():
            if b.is_floating_point():
                b.data = self.ema_bufs.views[name]
            else:
                b.data = self.ema_nbt[i:i + 1].view(b.shape)
                i += 1
        self.ema_projector = copy.deepcopy(self.projector).requires_grad_(False).eval()
        self.ema_projector.weight.data = self.pj_ema[:nm].view(1, nm, 1, 1)
        self.ema_projector.bias.data = self.pj_ema[nm:nm + 1]

    def step(self, x: torch.Tensor, gt_boxes: torch.Tensor, gt_masks: torch.Tensor, gt_cls: torch.Tensor) -> torch.Tensor:
        """One optimisation step on this rank's shard.  Returns the loss tuple of `_multitask_loss` as an 8-element device tensor view
        (total, seg, box, dfl, cls_det, img_cls, #positives, mean matched IoU) -- no host synchronisation.  With `instance_mask_weight` > 0
        the total includes `weight * mask_loss` and two elements are appended: mask_loss and its positive count.  With a region weight
        > 0 the total includes the weighted region terms and two more elements follow after everything else: dice, boundary."""
        loss = self.forward_backward(x, gt_boxes, gt_masks, gt_cls)
        self._clip_and_update()
        self.m.mark_weights_updated()                      # inference plans folded the old weights
        return loss

    def forward_backward(self, x: torch.Tensor, gt_boxes: torch.Tensor, gt_masks: torch.Tensor, gt_cls: torch.Tensor) -> torch.Tensor:
        """Forward, loss, backward and (with more than one rank) the gradient exchange: afterwards `self.grads` / `self.pj_grad` hold this
        step's (averaged) gradients.  No parameter is touched."""
        tp, lib, dev = self.tp, self.lib, self.dev
        tp.run_forward(x)
        nm = self.m.proto_ch
        region = self.seg_dice_weight > 0 or self.seg_boundary_weight > 0
        res, g, *seg_logits = multitask_loss([m.nchw() for m in tp.det_maps], tp.protos.nchw(), tp.logits, gt_boxes, gt_masks, gt_cls,
                                             self.projector.weight, self.projector.bias, with_grads=True, want_seg_logits=region,
                                             grad_out={"det_maps": [d.buf for d in tp.d_in["det"]], "img_logits": tp.d_in["logits"]}, **self.loss_kw)
        dseg = g["seg_logits"]
        if region:                   # ADDED to the BCE gradient in dseg: the projector's backward below then carries both
            reg = seg_region_loss(seg_logits[0], gt_masks.to(dev), bias=self.projector.bias, dice_weight=self.seg_dice_weight,
                                  boundary_weight=self.seg_boundary_weight, smooth=self.seg_dice_smooth, grad_out=dseg, accumulate=True)[0]
        assigned = None
        if self.det_loss == "tal":   # overwrites d_in["det"] whole
            r = task_aligned_det_loss([m.nchw() for m in tp.det_maps], gt_boxes, img_size=self.S, nc_det=self.loss_kw["nc_det"],
                                      reg_max=self.loss_kw["reg_max"], weights=self.tal_w, grad_out=[d.buf for d in tp.d_in["det"]],
                                      want_assignment=self.mask_assign == "tal", **self.tal_kw)
            tal = r[0]
            if self.mask_assign == "tal":
                assigned = r[2]
            wb, wd, wc = self.tal_w
            res = (res[0] + (wb * tal[0] + wd * tal[1] + wc * tal[2]), res[1], tal[0], tal[1], tal[2], res[5], tal[3], tal[4])
        mask = None
        if self.mask_w > 0:          # writes d_in["mc"] and d_in["protos"] whole; the projector's share is then ADDED to the latter
            mask = instance_mask_loss([m.nchw() for m in tp.det_maps], tp.mc, tp.protos.nchw(), gt_boxes, gt_masks, img_size=self.S,
                                      reg_max=self.loss_kw["reg_max"], iou_match_thresh=self.loss_kw["iou_match_thresh"], weight=self.mask_w,
                                      mc_layout="bAn", grad_out={"mc": tp.d_in["mc"], "protos": tp.d_in["protos"]}, assigned=assigned)[0]
        L.check(lib.mtbt_projector_backward(dseg.data_ptr(), tp.protos.ptr, self.pj.data_ptr(), tp.d_in["protos"].data_ptr(), tp.code, int(mask is not None),
                                            self.pj_grad.data_ptr(), self.pj_grad.data_ptr() + 4 * nm, 0, self.B, self.S // 4, self.S // 4, nm, self.S, self.S,
                                            self.pj_ws.data_ptr(), self.pj_ws.numel() * 4, L.stream(dev)), "mtbt_projector_backward")
        self._backward_and_exchange()
        if mask is not None:
            res = (res[0] + self.mask_w * mask[0],) + tuple(res[1:]) + mask
        if region:
            res = (res[0] + reg[2],) + tuple(res[1:]) + reg[:2]
        return torch.stack(res)

    def _backward_and_exchange(self):
        main = torch.cuda.current_stream(self.dev)
        if self.world == 1:
            self.tp.issue(self.bwd)
            return
        live = list(range(self.n_skip, len(self.grads.buckets)))
        if self.comm is None:
            self.tp.issue(self.bwd)
            for b in live:
                self._mean_over_ranks(self.grads.buckets[b])
            self._reduce_projector()
            return
        # The backward plan runs on several lanes (HIP streams) and the slots of one bucket are independent regions for its scheduler, so a
        # bucket's writers sit on SEVERAL lanes: every one of them is marked, Plan.run records one event per lane that carries a marked
        # launch (after that lane's last one), and the collective waits for ALL of those events.  (Round 2 marked only the bucket's
        # program-order-last writer: an earlier writer on another lane could still be running when the bucket was reduced.)
        marks, order = exchange_marks(self.writers, live)
        events = self.tp.issue(self.bwd, marks=marks)
        end = torch.cuda.Event()
        end.record(main)                       # behind the plan's join: every lane's work, for a bucket no recorded launch writes
        # buckets complete roughly in bucket order (reverse registration = backward order): ordered by their LATEST writer
        with torch.cuda.stream(self.comm):
            for b in order:
                evs = events.get(str(b))
                for ev in (evs if evs else [end]):
                    self.comm.wait_event(ev)
                self._mean_over_ranks(self.grads.buckets[b])
        main.wait_stream(self.comm)
        self._reduce_projector()

    def _reduce_projector(self):
        self._mean_over_ranks(self.pj_grad)

    def _mean_over_ranks(self, t: torch.Tensor):
        """Pre-scaled SUM = mean (what DDP hands the optimiser).  Backend "nccl" is RCCL over xGMI; the "gloo" rehearsal backend (several
        ranks sharing one GPU in the tests) may lack device-tensor collectives on this build and then stages through the host."""
        t.div_(self.world)
        if not self._host_staged:
            try:
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
                return
            except RuntimeError as e:
                if dist.get_backend(self.group) != "gloo":
                    raise
                self._note_host_staging(e)
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
        t.copy_(h)

    def _note_host_staging(self, err):
        """gloo rehearsal only: device-tensor collectives failed once, every later collective goes through the host.  Said ONCE, with the
        error that tripped it, so that a real failure in this mode does not hide behind the fallback."""
        self._host_staged = True
        if not self._host_staged_logged:
            self._host_staged_logged = True
            import warnings
            warnings.warn(f"TrainStep: gloo collective on a device tensor failed ({type(err).__name__}: {err}); staging every collective through "
                          "host memory from now on (rehearsal backend only -- RCCL errors are raised)")

    def sync_buffers(self, src: int = 0):
        """Rank `src`'s BatchNorm running statistics to every rank.  (torch DDP broadcasts buffers before EVERY forward; a train-mode
        forward never reads them, so doing it before validation / checkpointing is equivalent and costs nothing per step.)"""
        if self.world > 1:
            for buf in list(self.m.buffers()) + (list(self.ema_model.buffers()) if self.ema is not None else []):
                self._bcast(buf, src)
            if self.ema is not None:
                self.ema_model.mark_weights_updated()

    def _bcast(self, t: torch.Tensor, src: int):
        if not self._host_staged:
            try:
                dist.broadcast(t, src=src, group=self.group)
                return
            except RuntimeError as e:
                if dist.get_backend(self.group) != "gloo":
                    raise
                self._note_host_staging(e)
        h = t.cpu()
        dist.broadcast(h, src=src, group=self.group)
        t.copy_(h)

    def _clip_and_update(self):
        lib, s = self.lib, L.stream(self.dev)
        self.steps += 1
        live = list(range(self.n_skip, len(self.grads.buckets)))
        scale = None
        if self.clip_norm is not None:
            first = True
            for t in [self.grads.buckets[b] for b in live] + [self.pj_grad]:
                L.check(lib.mtbt_sumsq(t.data_ptr(), t.numel(), self.sq.data_ptr(), 0 if first else 1, self.sq_ws.data_ptr(), self.sq_ws.numel() * 4, s), "mtbt_sumsq")
                first = False
            L.check(lib.mtbt_clip_coef(self.sq.data_ptr(), float(self.clip_norm), self.coef.data_ptr(), self.gnorm.data_ptr(), s), "mtbt_clip_coef")
            scale = self.coef.data_ptr()
        targets = [(self.params.buckets[b], self.grads.buckets[b], self.m1[b], self.m2[b] if self.m2 else None) for b in live]
        targets.append((self.pj, self.pj_grad, self.pj_m, self.pj_v if self.opt == "adamw" else None))
        if self.ema is not None:
            self._update_with_ema(targets, [self.ema.buckets[b] for b in live] + [self.pj_ema], scale, s)
            return
        for p, g, m1, m2 in targets:
            if self.opt == "adamw":
                L.check(lib.mtbt_adamw_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), p.numel(), self.lr, self.betas[0], self.betas[1], self.eps,
                                            self.wd, self.steps, scale, s), "mtbt_adamw_step")
            else:
                L.check(lib.mtbt_sgd_step(p.data_ptr(), g.data_ptr(), m1.data_ptr(), p.numel(), self.lr, self.momentum, 0.0, self.wd, int(self.nesterov),
                                          self.steps, scale, s), "mtbt_sgd_step")

    def _update_with_ema(self, targets, emas, scale, s):
        """The optimiser launches of `_clip_and_update` through the `_ema` entry points (same parameters and moments, bit for bit, plus the
        average), then one launch for all floating-point buffers.  The unstepped leading buckets get no launch: their average stays
        equal to the parameters exactly."""
        lib = self.lib
        self.ema_updates += 1
        d = ema_decay_at(self.ema_updates, *self.ema_cfg)
        for (p, g, m1, m2), e in zip(targets, emas):
            if self.opt == "adamw":
                L.check(lib.mtbt_adamw_step_ema(p.data_ptr(), g.data_ptr(), m1.data_ptr(), m2.data_ptr(), e.data_ptr(), p.numel(), self.lr, self.betas[0],
                                                self.betas[1], self.eps, self.wd, self.steps, scale, d, s), "mtbt_adamw_step_ema")
            else:
                L.check(lib.mtbt_sgd_step_ema(p.data_ptr(), g.data_ptr(), m1.data_ptr(), e.data_ptr(), p.numel(), self.lr, self.momentum, 0.0, self.wd,
                                              int(self.nesterov), self.steps, scale, d, s), "mtbt_sgd_step_ema")
        for e, b in zip(self.ema_bufs.buckets, self.bufs.buckets):
            L.check(lib.mtbt_ema_update(e.data_ptr(), b.data_ptr(), b.numel(), d, s), "mtbt_ema_update")
        self.ema_nbt.copy_(self.nbt)                       # counters are copied, not averaged
        self.ema_model.mark_weights_updated()              # its inference plans folded the old averages

    # ------------------------------------------------------------------------------------------------------------------
    def _moment_views(self, buckets, pj):
        """{checkpoint name: view in the parameter's own torch shape} of one moment (flat buckets + the projector's flat buffer)."""
        nm = self.m.proto_ch
        out = {}
        for name, (b, o, k, shape) in self.params.where.items():
            out["net." + name] = self._gview[name](buckets[b][o:o + k].view(shape))
        out[PROJECTOR_KEYS[0]], out[PROJECTOR_KEYS[1]] = pj[:nm].view(1, nm, 1, 1), pj[nm:nm + 1]
        return out

    def _moments(self):
        slots = {"exp_avg": (self.m1, self.pj_m), "exp_avg_sq": (self.m2, self.pj_v)} if self.opt == "adamw" else {"momentum_buffer": (self.m1, self.pj_m)}
        return {slot: self._moment_views(b, pj) for slot, (b, pj) in slots.items()}

    def _live_tensors(self):
        """(`state_dict`, `ema_state_dict` | None) as {name: the live device tensor}."""
        sd = {"net." + k: v for k, v in self.m.state_dict(keep_vars=True).items()}
        sd[PROJECTOR_KEYS[0]], sd[PROJECTOR_KEYS[1]] = self.projector.weight, self.projector.bias
        if self.ema is None:
            return sd, None
        esd = dict(self.ema_model.state_dict(keep_vars=True))
        esd[PROJECTOR_KEYS[0]], esd[PROJECTOR_KEYS[1]] = self.ema_projector.weight, self.ema_projector.bias
        return sd, esd

    def state_dict(self) -> dict:
        """Everything needed to continue this step elsewhere, as one nested dict of CPU tensors, ints, floats and strings
        (`torch.load(..., weights_only=True)` reads it back):
          "state_dict"      parameters and buffers as `net.<name>` + `seg_proto_projector.weight / .bias` -- a Lightning checkpoint's names
                            (`checkpoints.strip_lightning_prefix` reads it);
          "ema_state_dict"  the same names without the `net.` prefix, from the averaged weights (only with `ema=`);
          "optimizer"       {name: {"exp_avg", "exp_avg_sq"}} or {name: {"momentum_buffer"}}, the names of "state_dict";
          "steps", "ema_updates", "lr", "optimizer_name", "det_loss", "mask_assign";
          "seg_dice_weight", "seg_boundary_weight", "seg_dice_smooth": the region weights at the time of saving, for the record only.
        Every tensor is keyed by parameter name and has the parameter's own shape, so the file does not depend on the bucket layout."""
        sd, esd = self._live_tensors()
        out = {"state_dict": {k: _cpu(v) for k, v in sd.items()}}
        if esd is not None:
            out["ema_state_dict"] = {k: _cpu(v) for k, v in esd.items()}
        opt = {}
        for slot, views in self._moments().items():
            for name, v in views.items():
                opt.setdefault(name, {})[slot] = _cpu(v)
        out.update(optimizer=opt, steps=int(self.steps), ema_updates=int(self.ema_updates), lr=float(self.lr), optimizer_name=str(self.opt),
                   det_loss=str(self.det_loss), mask_assign=str(self.mask_assign))
        # informational (the weights are attributes a schedule moves: loading checks none of them, and a state without them loads)
        out.update(seg_dice_weight=float(self.seg_dice_weight), seg_boundary_weight=float(self.seg_boundary_weight),
                   seg_dice_smooth=float(self.seg_dice_smooth))
        return out

    @torch.no_grad()
    def load_state_dict(self, state: dict):
        """Write a `state_dict()` into the existing storage, in place (the plans keep their pointers).  ValueError, before anything is
        written, for another optimiser, detection loss or mask assignment, names or shapes that do not match, or an EMA on one side only."""
        if not isinstance(state, dict) or "state_dict" not in state or "optimizer" not in state:
            raise ValueError("load_state_dict: not a TrainStep state (expected the keys of TrainStep.state_dict())")
        if state.get("optimizer_name") != self.opt:
            raise ValueError(f"load_state_dict: the state was saved by optimizer {state.get('optimizer_name')!r}, this step runs {self.opt!r}")
        if state.get("det_loss", "reference") != self.det_loss:
            raise ValueError(f"load_state_dict: the state was trained with det_loss {state.get('det_loss', 'reference')!r}, this step runs {self.det_loss!r}")
        if state.get("mask_assign", "iou") != self.mask_assign:
            raise ValueError(f"load_state_dict: the state was trained with mask_assign {state.get('mask_assign', 'iou')!r}, this step runs {self.mask_assign!r}")
        if ("ema_state_dict" in state) != (self.ema is not None):
            raise ValueError("load_state_dict: the state holds an EMA and this step keeps none (construct it with ema=...)" if self.ema is None
                             else "load_state_dict: this step keeps an EMA and the state holds none")
        sd, esd = self._live_tensors()
        moments = self._moments()
        pairs = []

        def match(what, dst, src):
            if not isinstance(src, dict) or set(src) != set(dst):
                odd = sorted(set(dst) ^ set(src if isinstance(src, dict) else ()))
                raise ValueError(f"load_state_dict: {what} names differ ({len(odd)}): {odd[:6]}")
            for k, t in dst.items():
                if not isinstance(src[k], torch.Tensor) or tuple(src[k].shape) != tuple(t.shape):
                    raise ValueError(f"load_state_dict: {what}[{k!r}] has shape {tuple(getattr(src[k], 'shape', ()))}, expected {tuple(t.shape)}")
                pairs.append((t, src[k]))

        match("state_dict", sd, state["state_dict"])
        if esd is not None:
            match("ema_state_dict", esd, state["ema_state_dict"])
        names = set(next(iter(moments.values())))
        if not isinstance(state["optimizer"], dict) or set(state["optimizer"]) != names:
            odd = sorted(names ^ set(state["optimizer"] if isinstance(state["optimizer"], dict) else ()))
            raise ValueError(f"load_state_dict: optimizer names differ ({len(odd)}): {odd[:6]}")
        for slot, views in moments.items():
            match(f"optimizer {slot}", views, {k: v.get(slot) if isinstance(v, dict) else None for k, v in state["optimizer"].items()})
        for dst, src in pairs:
            (dst.data if isinstance(dst, nn.Parameter) else dst).copy_(src)
        self.steps, self.ema_updates, self.lr = int(state["steps"]), int(state["ema_updates"]), float(state["lr"])
        self.m.mark_weights_updated()
        if self.ema is not None:
            self.ema_model.mark_weights_updated()

    def warmup_cosine_lr(self, base_lr: float, it: int, warmup_its: int, total_its: int, eta_min_ratio: float = 0.01, start_ratio: float = 0.0) -> float:
        """Per-ITERATION schedule: linear from `start_ratio * base_lr` (it = 0) to `base_lr` (it = warmup_its), then `cosine_lr`'s closed
        form over the remaining `total_its - warmup_its` iterations -- torch's SequentialLR([LinearLR, CosineAnnealingLR], [warmup_its])."""
        if it < warmup_its:
            self.lr = base_lr * (start_ratio + (1.0 - start_ratio) * it / warmup_its)
            return self.lr
        return self.cosine_lr(base_lr, it - warmup_its, total_its - warmup_its, eta_min_ratio)

    def cosine_lr(self, base_lr: float, epoch: int, t_max: int, eta_min_ratio: float = 0.01) -> float:
        """CosineAnnealingLR(T_max, eta_min = 0.01 * lr) in closed form (running_main_v3.py:742), applied per epoch."""
        eta_min = base_lr * eta_min_ratio
        self.lr = eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * epoch / t_max)) / 2
        return self.lr
