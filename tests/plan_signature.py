"""Canonical record of a launch plan (not a test): what `tests/test_cpu_plan_signature.py` hashes and compares with
`tests/golden/plan_signatures.json`.

A plan lowered on CPU tensors issues nothing, but every launch record is complete: the C symbol, its scalar arguments, its argument
blocks and the regions it reads and writes.  `plan_record` turns that into plain data that does not depend on where the allocator put
the buffers: every storage is named by the order of its first appearance in the plan, every pointer becomes (buffer index, byte offset).
Two lowerings that produce the same record issue the same launches with the same arguments on the same buffers.

Run as a script it prints the full record of one case, so that the records of two checkouts can be diffed:
    python tests/plan_signature.py                      # the case ids
    python tests/plan_signature.py canonical-bf16-merged
"""
import bisect
import contextlib
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_signatures.json")


class _Buffers:
    """Every storage a plan can point into, and the index each one gets when the record first meets it."""

    def __init__(self):
        self.spans = {}        # storage address -> bytes
        self.blocks = {}       # address of a ctypes argument block -> the block
        self.order = {}        # storage address -> index of first appearance
        self._starts = None

    def add(self, obj):
        if isinstance(obj, torch.Tensor):
            st = obj.untyped_storage()
            if st.nbytes():
                self.spans[st.data_ptr()] = max(self.spans.get(st.data_ptr(), 0), st.nbytes())
                self._starts = None
        elif isinstance(obj, nn.Module):
            for t in itertools.chain(obj.parameters(), obj.buffers()):
                self.add(t)
        elif isinstance(obj, (C.Structure, C.Array)):
            self.blocks[C.addressof(obj)] = obj
        elif isinstance(obj, (tuple, list)):
            for o in obj:
                self.add(o)
        elif hasattr(obj, "buf"):                      # engine.Act
            self.add(obj.buf)

    def index(self, base):
        return self.order.setdefault(base, len(self.order))

    def pointer(self, value, where):
        """A device pointer as [buffer index, byte offset]; None stays None."""
        if not value:
            return None
        if self._starts is None:
            self._starts = sorted(self.spans)
        k = bisect.bisect_right(self._starts, value) - 1
        base = self._starts[k] if k >= 0 else None
        if base is None or value >= base + self.spans[base]:
            raise LookupError(f"{where}: pointer {value:#x} lies in no buffer the plan keeps alive")
        return [self.index(base), value - base]

    def region(self, r, where):
        return [self.pointer(r[0], where)] + [int(v) for v in r[1:]]


def _scalar(v):
    if isinstance(v, C._SimpleCData):
        v = v.value
    return float(v).hex() if isinstance(v, float) else v


def _fields(block, bufs, where):
    """Every field of a ctypes argument block (nested blocks and arrays included)."""
    if isinstance(block, C.Array):
        if issubclass(block._type_, (C.Structure, C.Array)):
            return [_fields(b, bufs, where) for b in block]
        if block._type_ is C.c_void_p:
            return [bufs.pointer(v, where) for v in block]
        return [_scalar(v) for v in block]
    out = {}
    for name, typ in block._fields_:
        v = getattr(block, name)
        if typ is C.c_void_p:
            out[name] = bufs.pointer(v, f"{where}.{name}")
        elif isinstance(v, (C.Structure, C.Array)):
            out[name] = _fields(v, bufs, f"{where}.{name}")
        else:
            out[name] = _scalar(v)
    return out


def _argument(arg, typ, bufs, where, launch):
    if hasattr(arg, "_obj"):                           # ctypes.byref(block)
        return _fields(arg._obj, bufs, where)
    if typ is C.c_void_p:
        value = arg.value if isinstance(arg, C.c_void_p) else arg
        if value in bufs.blocks:                        # a batch: the array of argument blocks
            return _fields(bufs.blocks[value], bufs, where)
        if launch.fn.__name__ == "mtbt_weight_prep" and where.endswith("[0]"):
            # the table of prep descriptors is a byte tensor (a device buffer in a real plan): decoded, its pointers are arguments too
            from multitask_bonetumor_yolo_amd import _lib as L
            table = next(t for t in launch.keep if isinstance(t, torch.Tensor) and t.data_ptr() == value)
            raw = bytes(table.cpu().numpy())
            descs = (L.PrepDesc * (len(raw) // C.sizeof(L.PrepDesc))).from_buffer_copy(raw)
            return [bufs.pointer(value, where), _fields(descs, bufs, where)]
        return bufs.pointer(value, where)
    return _scalar(arg)


def plan_record(plan, roots=(), extra=None):
    """The canonical record of `plan` (engine.Plan).  `roots`: objects that own memory the plan points into without keeping it in a launch's
    `keep` (the model: parameters and BatchNorm buffers read in place; the training plan's scratch pool)."""
    bufs = _Buffers()
    bufs.add(list(roots))
    bufs.add(plan.consts)
    bufs.add(plan.pool.all)
    for l in plan.launches:
        bufs.add(list(l.keep))
    launches = []
    for i, l in enumerate(plan.launches):
        where = f"launch {i} {l.name}"
        types = list(l.fn.argtypes)
        assert len(types) == len(l.args) + 1, where     # (+ the stream, supplied by run())
        launches.append({
            "name": l.name, "fn": l.fn.__name__, "flops": float(l.flops).hex(), "bytes": float(l.bytes).hex(), "side": bool(l.side),
            "args": [_argument(a, t, bufs, f"{where} arg[{k}]", l) for k, (a, t) in enumerate(zip(l.args, types))],
            "reads": [bufs.region(r, where) for r in l.reads],
            "writes": [bufs.region(r, where) for r in l.writes],
        })
    sch = plan.schedule()
    rec = {"launches": launches, "dependencies": plan.dependencies(), "lane": list(sch.lane), "waits": [list(w) for w in sch.waits],
           "records": list(sch.records)}
    if extra:
        rec.update(extra)
    return rec


def compiled_record(model, c):
    """Record of an inference plan (`model._Compiled`)."""
    return plan_record(c.plan, roots=[model], extra={"det_marks": list(c.det_marks), "mask_marks": list(c.mask_marks),
                                                     "n_train_bns": len(c.train_bns)})


def digest(record) -> str:
    return hashlib.sha256(json.dumps(record, sort_keys=True).encode()).hexdigest()


# ---- the cases of the fixture ------------------------------------------------------------------------------------------------------------
OPTIONS = {"default": {}, "merged": {"HEADS_MERGED": "1"},
           "early": {"HEADS_EARLY": "1", "ADAPTOR_EARLY": "1", "SEG_GATE": "1", "NODE_FUSED": "1"}}
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}


def _variants():
    from multitask_bonetumor_yolo_amd import model as M
    return {"canonical": lambda: M.ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), "v2": lambda: M.ConvNeXtBiFPNYOLOv2(2, 2, pretrained_backbone=False),
            "v0": lambda: M.ConvNeXtBiFPNYOLOv0(2, 2)}


def inference_cases():
    """id -> (variant, dtype name, options name, heads in train mode, input shape)."""
    cases = {}
    small, big = (2, 3, 64, 64), (16, 3, 640, 640)
    for v in ("canonical", "v2", "v0"):
        for d in DTYPES:
            for o in OPTIONS:
                cases[f"{v}-{d}-{o}"] = (v, d, o, False, small)
    for v in ("canonical", "v2"):
        for d in DTYPES:
            cases[f"{v}-{d}-trainheads"] = (v, d, "default", True, small)
    for o in ("default", "merged"):
        cases[f"canonical-bf16-{o}-16x640"] = ("canonical", "bf16", o, False, big)
    return cases


def _training_case(variant, dtype, active=None, bn_eval=False, tail=False, **switches):
    """`active`: the outputs that carry a gradient (None: all five, and the entry holds the forward plan too); `bn_eval`: every BatchNorm2d
    in eval mode; `tail`: `tail_prefixes` = what the native training step passes; `switches`: module attributes of `train` for the lowering."""
    return {"variant": variant, "dtype": dtype, "active": active, "bn_eval": bn_eval, "tail": tail, "switches": switches}


SUBSETS = {"step": ("det", "logits", "protos"), "logits": ("logits",), "segmc": ("seg", "mc"), "protos": ("protos",)}
TRAINING_CASES = {
    "train-canonical-bf16": _training_case("canonical", "bf16"), "train-canonical-fp32": _training_case("canonical", "fp32"),
    "train-v0-fp32": _training_case("v0", "fp32"),
    "train-v2-fp32": _training_case("v2", "fp32"),
    "train-canonical-fp32-bneval": _training_case("canonical", "fp32", bn_eval=True),
    "train-canonical-bf16-tail": _training_case("canonical", "bf16", tail=True),
    "train-canonical-bf16-unfused": _training_case("canonical", "bf16", FUSED_BN_STATS=False, FUSED_TRAIN_MLP=False),
    **{f"train-canonical-bf16-{k}": _training_case("canonical", "bf16", active=a) for k, a in SUBSETS.items()}}


def make_model(variant, dtype, options=None, train_heads=False, train=False):
    from multitask_bonetumor_yolo_amd import model as M
    torch.manual_seed(0)
    m = M.init_synthetic_(_variants()[variant](), seed=0).eval()
    m.set_compute_dtype(DTYPES[dtype])
    if options:
        m.plan_options = dict(OPTIONS[options])
    if train:
        m.train()
    if train_heads:
        for h in (getattr(m, "detect", None), m.segment):
            if h is not None:
                h.train()
    return m


def lower_inference(model, shape):
    """The inference plan of `model` for an input of `shape`, lowered on CPU tensors."""
    from multitask_bonetumor_yolo_amd.engine import code_of
    from multitask_bonetumor_yolo_amd.model import _Lowering
    return _Lowering(model, shape, torch.device("cpu"), code_of(model.compute_dtype)).lower()


def inference_record(case_id):
    variant, dtype, options, train_heads, shape = inference_cases()[case_id]
    model = make_model(variant, dtype, options, train_heads)
    return compiled_record(model, lower_inference(model, shape))


@contextlib.contextmanager
def dry_lowering(**switches):
    """`train.DRY_LOWERING` on and the given module attributes of `train` set while a plan is lowered; restored afterwards."""
    from multitask_bonetumor_yolo_amd import train as T
    values = {"DRY_LOWERING": True, **switches}
    saved = {k: getattr(T, k) for k in values}
    for k, v in values.items():
        setattr(T, k, v)
    try:
        yield T
    finally:
        for k, v in saved.items():
            setattr(T, k, v)


def lower_training(case_id):
    """(model, `TrainPlan` at (2, 3, 64, 64)) of a training case, lowered on CPU tensors."""
    from multitask_bonetumor_yolo_amd.engine import code_of
    c = TRAINING_CASES[case_id]
    model = make_model(c["variant"], c["dtype"], train=True)
    if c["bn_eval"]:
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
    tail = ()
    if c["tail"]:
        from multitask_bonetumor_yolo_amd.trainstep import UNUSED_BY_THE_LOSS as tail
    with dry_lowering(**c["switches"]) as T:
        return model, T.TrainPlan(model, (2, 3, 64, 64), torch.device("cpu"), code_of(DTYPES[c["dtype"]]), tail_prefixes=tail)


def training_plan_record(model, tp, active=None, switches=None):
    """Record of `tp`'s backward plan for the outputs `active` (lowered here, under `switches`); of its forward plan with `active` None."""
    plan = tp.fwd
    if active is not None:
        with dry_lowering(**(switches or {})):
            plan = tp.backward_plan(active)
    roots = [model, tp.x, tp.ws.small, tp.ws.big, tp.arena.buckets, tp.fwd.pool.all, tp.fwd.consts]
    return plan_record(plan, roots)


def training_records(case_id):
    """The records of a training case: [forward, backward for all outputs], or [backward] alone for a case that names its active outputs."""
    model, tp = lower_training(case_id)
    active, switches = TRAINING_CASES[case_id]["active"], TRAINING_CASES[case_id]["switches"]
    if active is not None:
        return [training_plan_record(model, tp, active, switches)]
    outputs = tp.OUT_NAMES if tp.det_maps is not None else tuple(n for n in tp.OUT_NAMES if n != "det")
    return [training_plan_record(model, tp), training_plan_record(model, tp, outputs, switches)]


def case_entry(case_id):
    """What the fixture holds for one case: launch count(s) and digest(s)."""
    if case_id in TRAINING_CASES:
        recs = training_records(case_id)
        return {"launches": [len(r["launches"]) for r in recs], "sha256": [digest(r) for r in recs]}
    rec = inference_record(case_id)
    return {"launches": len(rec["launches"]), "sha256": digest(rec)}


def all_case_ids():
    return list(inference_cases()) + list(TRAINING_CASES)


if __name__ == "__main__":
    for k in [k for k in os.environ if k.startswith("MTBT_")]:
        del os.environ[k]
    if len(sys.argv) < 2:
        print("\n".join(all_case_ids()))
    else:
        cid = sys.argv[1]
        rec = training_records(cid) if cid in TRAINING_CASES else inference_record(cid)
        json.dump(rec, sys.stdout, indent=1, sort_keys=True)
        print()
