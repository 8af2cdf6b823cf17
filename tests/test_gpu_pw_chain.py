"""mtbt_pw_chain_nhwc (two chained 1x1 convolutions in one launch, plan option PW_CHAIN) is BIT-IDENTICAL to the two mtbt_conv2d_nhwc launches
it replaces: kernel level on ragged / multi-tile pixel counts and sliced destinations, model level on the canonical model (eager and graph)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd.engine import Act, Plan

DEV = "cuda:0"
SENTINEL = -77.0          # exact in bf16 / fp16 / fp32
CH = 256
SHAPES = [(1, 5, 7), (2, 9, 8), (1, 16, 16)]      # 35 px: one ragged tile; 144 px: two whole 64-pixel tiles + a ragged one; 256 px: whole tiles only
FAMILIES = {"k256": (256, False), "k2": (2, True), "k32": (32, True)}       # K, fp32 output
LAYOUTS = [None, (512, 0), (512, 128)]            # dense, or (pixel pitch, channel offset)
TAIL = 8                                           # pixel rows behind the last pixel that must stay untouched
# from 65 536 pixels a workgroup runs TWO 64-pixel tiles: 65 571 = 512 x 128 + 35 (last workgroup: a ragged first tile, an empty second one),
# 65 786 = 513 x 128 + 122 (a whole first tile, a ragged second one)
BIG_SHAPES = [(1, 33, 1987), (1, 259, 254)]


def operands(dtype, K, shape, seed):
    """x, W1, shift1, W2, shift2.  The pre-activation of t has a standard deviation of ~2 and a shift of ~1: t spans both signs, well inside
    and outside +-1, so ELU (exponential below 0, both of its branches around -0.03) and SiLU run off their linear parts."""
    g = torch.Generator().manual_seed(seed)
    N, H, W = shape
    x = torch.randn(N, H, W, CH, generator=g).to(dtype).to(DEV)
    w1 = (torch.randn(CH, CH, generator=g) * 0.125).to(dtype).to(DEV)
    s1 = torch.randn(CH, generator=g).to(DEV)
    w2 = (torch.randn(K, CH, generator=g) * 0.08).to(dtype).to(DEV)
    s2 = torch.randn(K, generator=g).to(DEV)
    return x, w1, s1, w2, s2


def destination(shape, K, out_dtype, layout):
    N, H, W = shape
    ld, c0 = layout if layout else (K, 0)
    buf = torch.full(((N * H * W + TAIL) * ld,), SENTINEL, dtype=out_dtype, device=DEV)
    return buf, Act(buf, c0, N, H, W, K, ld, H * W * ld)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES + BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_chain_equals_the_two_launches(family, shape, dtype):
    K, f32 = FAMILIES[family]
    act1, act2 = (L.ACT_SILU, L.ACT_NONE) if f32 else (L.ACT_ELU, L.ACT_SILU)      # class branch / BiFPN node -> C2f cv1
    out_dtype = torch.float32 if f32 else dtype
    x, w1, s1, w2, s2 = operands(dtype, K, shape, seed=1000 + 10 * (SHAPES + BIG_SHAPES).index(shape) + len(family))
    xa = Act.of(x)
    N, H, W = shape
    npix = N * H * W
    p = Plan(torch.device(DEV))
    t = p.new(N, H, W, CH, xa.code)
    p.conv(xa, w1, t, shift=s1, act=act1, name="first")
    refs, gots = [], []
    layouts = LAYOUTS if shape in SHAPES else [None, (512, 128)]
    for layout in layouts:
        rbuf, ry = destination(shape, K, out_dtype, layout)
        p.conv(t, w2, ry, shift=s2, act=act2, name="second")
        gbuf, gy = destination(shape, K, out_dtype, layout)
        a = p.pw_chain_args(xa, w1, s1, act1, w2, s2, act2, gy, any_size=True)      # (the small maps are below the library's pixel-count rule)
        assert a is not None, (family, shape, layout)
        p.pw_chain(a, xa, w1, s1, w2, s2, gy, name="chain")
        refs.append(rbuf)
        gots.append(gbuf)
    p.run()
    torch.cuda.synchronize()
    tf = t.buf.float()
    # the intermediate really leaves the activations' linear parts: large positive values, ELU's exponential tail (below -0.5) and both of its
    # branches around -0.03, SiLU's trough (its minimum is -0.278)
    assert (tf > 1.5).any() and ((tf > -0.03) & (tf < 0)).any() and (tf < (-0.5 if act1 == L.ACT_ELU else -0.2)).any()
    for layout, rbuf, gbuf in zip(layouts, refs, gots):
        ld, c0 = layout if layout else (K, 0)
        assert torch.equal(gbuf, rbuf), (layout, (gbuf.float() - rbuf.float()).abs().max().item())
        rows = gbuf.view(npix + TAIL, ld)
        assert (rows[:npix, c0:c0 + K] != SENTINEL).any()
        assert (rows[:npix, :c0] == SENTINEL).all() and (rows[:npix, c0 + K:] == SENTINEL).all()      # channels outside the slice
        assert (rows[npix:] == SENTINEL).all()                                                           # nothing past the last pixel


def test_library_declines_what_it_has_no_kernel_for():
    """The no-launch query and the entry point agree: other widths, activations, dtypes and misaligned slices are refused with the library's
    error codes, nothing is launched."""
    lib = L.load()
    x, w1, s1, w2, s2 = operands(torch.bfloat16, 256, (1, 5, 7), seed=5)
    buf, y = destination((1, 5, 7), 256, torch.bfloat16, None)
    p = Plan(torch.device(DEV))
    import ctypes as C
    assert p.pw_chain_args(Act.of(x), w1, s1, L.ACT_ELU, w2, s2, L.ACT_SILU, y) is None            # 35 pixels: the two launches are advised
    good = p.pw_chain_args(Act.of(x), w1, s1, L.ACT_ELU, w2, s2, L.ACT_SILU, y, any_size=True)
    assert good is not None and lib.mtbt_pw_chain_supported(C.byref(good)) == 2
    for field, value in (("C", 128), ("M", 128), ("K", 128), ("act1", L.ACT_GELU), ("act2", L.ACT_GELU), ("dtype", L.F32), ("pixels", 0),
                         ("y_pixel_stride", 255), ("y_pixel_stride", 260), ("y", y.ptr + 2)):
        a = L.PwChainArgs.from_buffer_copy(good)
        setattr(a, field, value)
        assert lib.mtbt_pw_chain_supported(C.byref(a)) == 0, field
        assert lib.mtbt_pw_chain_nhwc(C.byref(a), None) in (-1, -2), field
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


@pytest.fixture(scope="module")
def model_and_input():
    from multitask_bonetumor_yolo_amd import calibrate_synthetic_heads_, init_synthetic_
    from multitask_bonetumor_yolo_amd.model import ConvNeXtBiFPNYOLO
    torch.manual_seed(21)
    hip = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(DEV).eval()
    x = torch.rand(2, 3, 160, 160, generator=torch.Generator().manual_seed(22)).to(DEV)      # P3 / P4 / P5 = 20^2, 10^2, 5^2: P5 is one ragged tile
    hip.set_compute_dtype(torch.float32)
    calibrate_synthetic_heads_(hip, x)
    hip.set_compute_dtype(torch.bfloat16)
    return hip, x


def _with_option(hip, value):
    hip.plan_options = {"PW_CHAIN": value}
    hip.__dict__.pop("_plans", None)


def _flat(out):
    feats, mc, protos = out["segment_protos"]
    return list(out["detect_features"]) + list(feats) + [mc, protos, out["img_cls_logits"], out["segment_preds_cat"], out["detect_preds_cat"]]


def test_model_outputs_do_not_change(model_and_input):
    """"1": the sites the library advises (at this size the class chains; the neck's maps are below its pixel-count rule); "2": every site it has a
    kernel for -- the 5 x 5 map of P5 is a single ragged tile."""
    hip, x = model_and_input
    res = {}
    try:
        for v in ("0", "1", "2"):
            _with_option(hip, v)
            with torch.no_grad():
                out = [t.clone() for t in _flat(hip(x, "infer"))]
            fwd, det = hip.infer_and_detect(x, 160)
            torch.cuda.synchronize()
            names = [l.name for l in hip.compile(x).plan.launches]
            res[v] = (out, {k: det[k].clone() for k in ("keep_idx", "scores", "boxes", "masks", "counts")}, names)
    finally:
        hip.__dict__.pop("plan_options", None)
        hip.__dict__.pop("_plans", None)
    assert len(res["0"][2]) - len(res["1"][2]) == 6 and len(res["0"][2]) - len(res["2"][2]) == 14
    assert sum(n.endswith("_conv+cf.cv1") for n in res["2"][2]) == 8 and sum(n.endswith(".1.1+2") for n in res["2"][2]) == 6
    assert not any("+" in n.split(".")[-1] and ("cf.cv1" in n or n.endswith(".1.1+2")) for n in res["0"][2])
    assert int(res["0"][1]["counts"].sum()) > 0
    for v in ("1", "2"):
        assert len(res["0"][0]) == len(res[v][0])
        for a, b in zip(res["0"][0], res[v][0]):
            assert torch.equal(a, b)
        for k in ("keep_idx", "scores", "boxes", "masks"):
            assert torch.equal(res["0"][1][k], res[v][1][k]), (v, k)


def test_graph_replay_with_the_option_equals_eager(model_and_input):
    from multitask_bonetumor_yolo_amd.graphed import GraphedInference
    hip, x = model_and_input
    try:
        _with_option(hip, "2")
        fwd, det = hip.infer_and_detect(x, 160)
        torch.cuda.synchronize()
        ref = [t.clone() for t in (fwd["segment_preds_cat"], fwd["detect_preds_cat"], fwd["segment_protos"][2], fwd["img_cls_logits"],
                                   det["keep_idx"], det["masks"])]
        g = GraphedInference(hip, x, 160)
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
        got = [g.fwd["segment_preds_cat"], g.fwd["detect_preds_cat"], g.fwd["segment_protos"][2], g.fwd["img_cls_logits"], g.out["keep_idx"],
               g.out["masks"]]
        assert all(torch.equal(a, b) for a, b in zip(ref, got))
        del g
    finally:
        hip.__dict__.pop("plan_options", None)
        hip.__dict__.pop("_plans", None)
