"""GPU checks of the batched convolution launch (mtbt_conv2d_nhwc_batch), the depth-multiplier depthwise entry (mtbt_dwconv3x3_mult_nhwc)
and the merged-heads inference plan (plan option HEADS_MERGED), each against the launches they replace."""
import pytest
import torch

from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, ConvNeXtBiFPNYOLOv2
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd.engine import Act, Plan, code_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# the tolerance tests/test_gpu_kernels.py holds the conv kernels to against the reference, per dtype (only where bit-equality is not claimed)
TOL = {torch.float32: 1e-3, torch.bfloat16: 2e-2, torch.float16: 2e-2}
ROW_REUSE = 1 << 25


def hint(tc, tp):
    return (tc << 16) | tp


def run(plan):
    plan.run(stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def conv_pair(dtype, n, k, N, H, W, Cin, K, act, f32_out, tile_hint, policy=0):
    """n equal convolutions over channel slices of one input buffer, once as n single calls and once as one batch, into buffers filled with
    a sentinel.  Outputs: channel slices of one [.., n*K + 8] buffer, or (fp32 head maps) channels [0, K) / [64, 64+K) of n maps of pitch 68."""
    g = torch.Generator().manual_seed(1000 * n + 10 * H + k + Cin)
    x = torch.randn(N, H, W, n * Cin, generator=g).to(DEV, dtype)
    ws = [(torch.randn(K, k * k * Cin, generator=g) / (k * k * Cin) ** 0.5).to(DEV, dtype) for _ in range(n)]
    shs = [torch.randn(K, generator=g).to(DEV) for _ in range(n)]
    xa = Act.of(x)
    results = []
    for batched in (False, True):
        if f32_out:
            bufs = [torch.full((N, H, W, 68), 7.0, dtype=torch.float32, device=DEV) for _ in range(n)]
            c0 = 0 if K == 64 else 64
            ys = [Act(b, c0, N, H, W, K, 68, H * W * 68) for b in bufs]
        else:
            bufs = [torch.full((N, H, W, n * K + 8), 7.0, dtype=dtype, device=DEV)]
            ys = [Act.of(bufs[0]).slice(j * K, K) for j in range(n)]
        p = Plan(torch.device(DEV))
        members = [(xa.slice(j * Cin, Cin), ws[j], ys[j], shs[j]) for j in range(n)]
        kw = dict(R=k, S=k, pad=k // 2, act=act, tile_hint=tile_hint, policy=policy)
        if batched:
            p.conv_batch(members, **kw)
            assert len(p.launches) == 1
        else:
            for xm, w, y, sh in members:
                p.conv(xm, w, y, shift=sh, **kw)
        run(p)
        results.append([b.clone() for b in bufs])
    return results


# (n, k, N, H, W, Cin, K, act, fp32 output, {dtype class: tile hint}) -- the hint is forced on BOTH sides so that kernel and K-step agree
SAME_TILE = [
    # row 3 of the merged heads: three 3x3 64 -> 64 over slices of one 192-channel buffer (80^2: row-reuse direct kernel; else implicit GEMM)
    (3, 3, 2, 80, 80, 64, 64, L.ACT_SILU, False, ROW_REUSE),
    (3, 3, 2, 40, 40, 64, 64, L.ACT_SILU, False, hint(64, 64)),
    (3, 3, 2, 20, 20, 64, 64, L.ACT_SILU, False, hint(64, 64)),
    # rows 4 / 6: two 1x1 256 -> 256 over slices of 512-channel buffers, on each tile the batch chooser can pick
    (2, 1, 2, 80, 80, 256, 256, L.ACT_SILU, False, hint(128, 128)),
    (2, 1, 2, 40, 40, 256, 256, L.ACT_SILU, False, hint(128, 64)),
    (2, 1, 2, 20, 20, 256, 256, L.ACT_SILU, False, hint(64, 64)),
    # row 7: two 1x1 64 -> 64 into fp32 maps of pitch 68
    (2, 1, 2, 80, 80, 64, 64, L.ACT_NONE, True, hint(64, 64)),
    (2, 1, 2, 40, 40, 64, 64, L.ACT_NONE, True, hint(64, 64)),
    (2, 1, 2, 20, 20, 64, 64, L.ACT_NONE, True, hint(64, 64)),
    # row 8: two 1x1 256 -> 2 into channels 64.. of the maps: implicit GEMM 32x64 (what fp32 mode runs), and below the streaming kernel
    (2, 1, 2, 80, 80, 256, 2, L.ACT_NONE, True, hint(32, 64)),
    (2, 1, 2, 20, 20, 256, 2, L.ACT_NONE, True, hint(32, 64)),
    # one member; pixel counts that are no multiple of the tile (63 and 126 pixels)
    (1, 3, 2, 20, 20, 64, 64, L.ACT_SILU, False, hint(64, 64)),
    (1, 1, 2, 40, 40, 256, 256, L.ACT_SILU, False, hint(128, 128)),
    (2, 1, 1, 9, 7, 64, 64, L.ACT_NONE, False, hint(64, 64)),
    (3, 3, 2, 9, 7, 64, 64, L.ACT_SILU, False, hint(64, 64)),
    (2, 3, 1, 16, 32, 128, 96, L.ACT_SILU, False, ROW_REUSE),       # direct kernel, ragged channel tiles (policy bit 5: 64-channel tiles)
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", SAME_TILE, ids=lambda c: f"n{c[0]}_k{c[1]}_{c[3]}x{c[4]}_{c[5]}to{c[6]}{'_f32' if c[8] else ''}")
def test_batch_equals_single_calls_on_the_same_tile(dtype, cfg):
    """mtbt_conv2d_nhwc_batch against n calls of mtbt_conv2d_nhwc with the same tile forced on both: BIT-IDENTICAL buffers (outputs and the
    sentinel around them) -- every output element runs the same K loop and epilogue, the batch only selects pointers by blockIdx.y."""
    n, k, N, H, W, Cin, K, act, f32, th = cfg
    single, batch = conv_pair(dtype, n, k, N, H, W, Cin, K, act, f32, th, policy=32 if (th == ROW_REUSE and K >= 96) else 0)
    for a, b in zip(single, batch):
        assert torch.equal(a, b)
    assert any((a != 7.0).any().item() for a in single)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("H", [80, 40, 20])
def test_batch_streaming_head_conv(dtype, H):
    """Row 8 in the 16-bit modes: the two class convs on the streaming kernel, batch against single calls, bit-identical."""
    single, batch = conv_pair(dtype, 2, 1, 2, H, H, 256, 2, L.ACT_NONE, True, 0)
    for a, b in zip(single, batch):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cfg", [c for c in SAME_TILE if c[0] > 1 and c[2] == 2], ids=lambda c: f"n{c[0]}_k{c[1]}_{c[3]}x{c[4]}_{c[5]}to{c[6]}{'_f32' if c[8] else ''}")
def test_batch_heuristic_choice_close_to_single_calls(dtype, cfg):
    """No hint: the batch may run another tile than a single call would; the results agree within the per-dtype tolerance of the kernel tests."""
    n, k, N, H, W, Cin, K, act, f32, _ = cfg
    single, batch = conv_pair(dtype, n, k, N, H, W, Cin, K, act, f32, 0)
    for a, b in zip(single, batch):
        d = (a.float() - b.float()).abs().max().item()
        print(f"heuristic batch vs single, {dtype}, {cfg[:7]}: max |diff| = {d:.3e}")
        assert d < TOL[dtype], d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [80, 40, 20])
@pytest.mark.parametrize("act", [L.ACT_SILU, L.ACT_NONE, L.ACT_ELU])
def test_dwconv_multiplier_equals_two_depthwise_calls(dtype, H, act):
    """mtbt_dwconv3x3_mult_nhwc, M = 2, C = 256: channels [m*C, (m+1)*C) are bit-identical to mtbt_dwconv_nhwc on the m-th block; M = 1 is
    the existing entry."""
    g = torch.Generator().manual_seed(H + act)
    N, Cc = 2, 256
    x = Act.of(torch.randn(N, H, H, Cc, generator=g).to(DEV, dtype))
    w = (torch.randn(9, 2 * Cc, generator=g) / 3).to(DEV, dtype)
    sc, sh = (torch.rand(2 * Cc, generator=g) + 0.5).to(DEV), (torch.randn(2 * Cc, generator=g) * 0.1).to(DEV)
    p = Plan(torch.device(DEV))
    y2 = Act.of(torch.full((N, H, H, 2 * Cc), 7.0, dtype=dtype, device=DEV))
    p.dwconv(x, w, y2, 3, scale=sc, shift=sh, act=act)
    ys = []
    for m in range(2):
        ys.append(Act.of(torch.full((N, H, H, Cc), 7.0, dtype=dtype, device=DEV)))
        p.dwconv(x, w[:, m * Cc:(m + 1) * Cc].contiguous(), ys[m], 3, scale=sc[m * Cc:(m + 1) * Cc].contiguous(), shift=sh[m * Cc:(m + 1) * Cc].contiguous(), act=act)
    y1 = torch.full((N, H, H, Cc), 7.0, dtype=dtype, device=DEV)
    lib = p.lib
    run(p)
    rc = lib.mtbt_dwconv3x3_mult_nhwc(x.ptr, w[:, :Cc].contiguous().data_ptr(), sc[:Cc].contiguous().data_ptr(), sh[:Cc].contiguous().data_ptr(), act,
                                      y1.data_ptr(), N, H, H, Cc, 1, code_of(dtype), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert p.launches[0].fn is lib.mtbt_dwconv3x3_mult_nhwc
    for m in range(2):
        assert torch.equal(y2.buf[..., m * Cc:(m + 1) * Cc], ys[m].buf)
    assert torch.equal(y1, ys[0].buf) and torch.isfinite(y2.buf.float()).all()


# ---- model level ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def calibrated(cls):
    from multitask_bonetumor_yolo_amd import calibrate_synthetic_heads_, init_synthetic_
    if cls not in _MODELS:
        torch.manual_seed(31)
        m = init_synthetic_(cls(2, 2, pretrained_backbone=False)).to(DEV).eval()
        m.set_compute_dtype(torch.float32)
        calibrate_synthetic_heads_(m, torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(32)).to(DEV))
        _MODELS[cls] = m
    return _MODELS[cls]


def flat_outputs(out):
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in flat_outputs(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for v in out for t in flat_outputs(v)]
    return [out] if isinstance(out, torch.Tensor) else []


def both_plans(model, x, S):
    res = {}
    for opt in ("0", "1"):
        model.plan_options = {"HEADS_MERGED": opt}
        with torch.no_grad():
            fwd = [t.clone() for t in flat_outputs(model(x, "infer"))]
            _, det = model.infer_and_detect(x, S, masks=False)
        torch.cuda.synchronize()
        res[opt] = (fwd, {k: det[k].clone() for k in ("boxes", "scores", "labels", "counts", "keep_idx")})
    model.__dict__.pop("plan_options")
    return res["0"], res["1"]


@pytest.mark.parametrize("cls", [ConvNeXtBiFPNYOLO, ConvNeXtBiFPNYOLOv2], ids=["canonical", "v2"])
@pytest.mark.parametrize("S", [256, 640])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_merged_heads_compute_what_the_separate_heads_compute(cls, S, dtype):
    """forward(x, "infer") and infer_and_detect with plan_options = {"HEADS_MERGED": "1"} against "0" on the same calibrated synthetic weights,
    batch 2.  fp32: every output within 1e-3 (max abs) of the unmerged plan's; bf16: against the unmerged bf16 plan (the same rounding points).
    Bit-identical maps are the expected case (each output element runs the separate lowering's K loop); whether they are has not been
    measured on an MI355X yet -- the test prints the per-output differences before it asserts."""
    model = calibrated(cls)
    model.set_compute_dtype(dtype)
    x = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(S)).to(DEV)
    try:
        (f0, d0), (f1, d1) = both_plans(model, x, S)
    finally:
        model.set_compute_dtype(torch.float32)
    assert len(f0) == len(f1) and len(f0) >= 8
    diffs = [(a.float() - b.float()).abs().max().item() for a, b in zip(f0, f1)]
    identical = all(torch.equal(a, b) for a, b in zip(f0, f1))
    print(f"merged vs separate heads, {cls.__name__}, {S}, {dtype}: identical={identical}, max |diff| per output = {['%.2e' % d for d in diffs]}, "
          f"kept {d0['counts'].tolist()} / {d1['counts'].tolist()}")
    assert int(d0["counts"].sum()) > 0
    if dtype == torch.float32:
        assert max(diffs) < 1e-3, diffs
    else:
        assert identical, diffs
    if identical:
        for k in d0:
            assert torch.equal(d0[k], d1[k]), k
    else:   # the comparison of tests/test_gpu_model.py::test_bf16_post_process_agrees_with_fp32_on_calibrated_heads, with its threshold
        from multitask_bonetumor_yolo_amd.metrics import box_iou_xyxy
        hit = tot = 0
        for b in range(x.shape[0]):
            n0, n1 = int(d0["counts"][b]), int(d1["counts"][b])
            assert n0 > 0 and n1 > 0
            iou = box_iou_xyxy(d1["boxes"][b, :n1].cpu().numpy(), d0["boxes"][b, :n0].cpu().numpy())
            hit += int((iou.max(axis=1) >= 0.7).sum()) + int((iou.max(axis=0) >= 0.7).sum())
            tot += n0 + n1
        assert hit / tot >= 0.75, hit / tot


@pytest.mark.parametrize("cls,fewer", [(ConvNeXtBiFPNYOLO, 30), (ConvNeXtBiFPNYOLOv2, 6)], ids=["canonical", "v2"])
def test_merged_plan_launch_counts(cls, fewer):
    """19 -> 9 launches per level (v2, Segment alone: 11 -> 9); a head BatchNorm in training mode keeps the separate lowering completely."""
    model = calibrated(cls)
    x = torch.rand(2, 3, 256, 256, device=DEV)

    def names(opt):
        model.plan_options = {"HEADS_MERGED": opt}
        return [l.name for l in model.compile(x).plan.launches]
    try:
        sep, mer = names("0"), names("1")
        assert len(sep) - len(mer) == fewer
        batches = [n for n in mer if " + " in n]
        assert len(batches) == (8 if fewer == 30 else 2) * 3
        model.segment.cv4[1][0].bn.train()
        sep_t, mer_t = names("0"), names("1")
        assert len(sep_t) - len(mer_t) == fewer * 2 // 3          # level 1 falls back, the other two stay merged
        for h in (model.segment,):
            for m in h.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.train()
        assert names("0") == names("1")
    finally:
        model.eval()
        model.__dict__.pop("plan_options", None)


def test_graphed_inference_replays_the_merged_plan():
    """GraphedInference captures the merged plan once and replays it three times; the outputs equal the eager merged run."""
    from multitask_bonetumor_yolo_amd.graphed import GraphedInference
    model = calibrated(ConvNeXtBiFPNYOLO)
    model.set_compute_dtype(torch.bfloat16)
    model.plan_options = {"HEADS_MERGED": "1"}
    try:
        x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(5)).to(DEV)
        with torch.no_grad():
            fwd, det = model.infer_and_detect(x, 256)
        torch.cuda.synchronize()
        ref = [t.clone() for t in (fwd["detect_preds_cat"], fwd["segment_preds_cat"], fwd["segment_protos"][2], det["keep_idx"], det["counts"], det["masks"])]
        g = GraphedInference(model, x, 256)
        assert any(" + " in l.name for l in g._compiled.plan.launches)
        for _ in range(3):
            out = g.replay()
            torch.cuda.synchronize()
            got = [g.fwd["detect_preds_cat"], g.fwd["segment_preds_cat"], g.fwd["segment_protos"][2], out["keep_idx"], out["counts"], out["masks"]]
            assert all(torch.equal(a, b) for a, b in zip(ref, got))
    finally:
        model.__dict__.pop("plan_options", None)
        model.set_compute_dtype(torch.float32)
