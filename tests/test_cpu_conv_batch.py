"""CPU checks of the batched convolution entry points, the depth-multiplier depthwise entry, `Plan.conv_batch` and the host-side weight
packing of the merged-heads lowering (plan option HEADS_MERGED).  Nothing here launches a kernel."""
import ctypes as C
import dataclasses

import pytest
import torch

import kernel_reference as KR
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

EINVAL = -1
# what the batched kernels are instantiated for (conv_batch_<dtype>.hip, pw_stream.hip): (kernel, channel tile, pixel tile, flag)
BATCH_SET = {(0, 64, 64, 1), (0, 128, 128, 1), (0, 128, 64, 1), (0, 32, 64, 1), (1, 64, 256, 0)}


def in_batch_set(choice):
    return tuple(choice) in BATCH_SET or (choice[0] == 2 and choice[1] <= 32 and choice[2] == 128)


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def head_args(N, H, Cin, K, k=1, act=L.ACT_SILU, dtype=L.BF16, out_dtype=None, ldx=None, ldy=None, x=0x100000, y=0x4000000, policy=0, hint=0):
    """Argument block of one head conv as engine.Plan fills it (fake, aligned pointers: the queries dereference nothing)."""
    a = L.ConvArgs()
    a.x, a.w, a.y, a.shift = x, 0x2000000, y, 0x3000000
    pad = k // 2
    a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad, a.Ho, a.Wo = N, H, H, Cin, K, k, k, 1, pad, H, H
    ldx, ldy = ldx or Cin, ldy or K
    a.x_pixel_stride, a.x_batch_stride, a.y_pixel_stride, a.y_batch_stride = ldx, H * H * ldx, ldy, H * H * ldy
    a.dtype, a.out_dtype, a.act, a.out_mode = dtype, dtype if out_dtype is None else out_dtype, act, L.OUT_NHWC
    a.policy, a.tile_hint = policy, hint
    return a


def batch_of(members):
    arr = (L.ConvArgs * len(members))()
    for i, m in enumerate(members):
        C.memmove(C.byref(arr, i * C.sizeof(L.ConvArgs)), C.byref(m), C.sizeof(L.ConvArgs))
    return arr


def batch_choice(lib, members):
    out = (C.c_int32 * 4)()
    rc = lib.mtbt_conv_batch_kernel_choice(batch_of(members), len(members), out)
    return rc, tuple(out)


def slices(n, width, **kw):
    """n members reading / writing channel slices of one [.., n * width] buffer each."""
    es = 4 if kw.get("dtype") == L.F32 else 2
    oes = 4 if kw.get("out_dtype", kw.get("dtype")) == L.F32 else 2
    return [head_args(x=0x100000 + j * kw["Cin"] * es, y=0x4000000 + j * width * oes, ldx=n * kw["Cin"], ldy=n * width, **kw) for j in range(n)]


def test_symbols_and_abi(lib):
    """The three additive symbols exist with the documented prototypes; the ABI version and the argument-block sizes did not move."""
    for name, nargs in (("mtbt_conv2d_nhwc_batch", 3), ("mtbt_conv_batch_kernel_choice", 3), ("mtbt_dwconv3x3_mult_nhwc", 13)):
        assert hasattr(lib, name)
        assert len(L.SYMBOLS[name][1]) == nargs and L.SYMBOLS[name][0] is C.c_int
    assert lib.mtbt_abi_version() == 5
    mirrors = [L.ConvArgs, L.FuseArgs, L.DecodeArgs, L.MaskArgs, L.LossArgs, L.PrepDesc, L.RawImage, L.UpconvArgs, L.NodeArgs, L.BoxEvalArgs]
    for which, st in enumerate(mirrors):
        assert lib.mtbt_sizeof_args(which) == C.sizeof(st), which
    assert lib.mtbt_sizeof_args(len(mirrors)) == -1                 # no new argument block


def test_batch_argument_checks(lib):
    """Every MTBT_EINVAL case of mtbt_conv2d_nhwc_batch returns before a launch (the valid case is only queried: no device here)."""
    def run(members, n=None):
        return lib.mtbt_conv2d_nhwc_batch(batch_of(members), len(members) if n is None else n, None)
    ok = lambda: slices(2, 64, N=2, H=20, Cin=64, K=64, k=3)
    assert batch_choice(lib, ok())[0] == 0
    assert run(ok(), 0) == EINVAL and run(ok() * 5, 9) == EINVAL and lib.mtbt_conv2d_nhwc_batch(None, 1, None) == EINVAL
    for field, value in (("K", 32), ("C", 128), ("H", 24), ("act", L.ACT_NONE), ("out_dtype", L.F32), ("dtype", L.F16), ("tile_hint", (64 << 16) | 64),
                         ("policy", 0x100 | 7 | 64), ("stride", 2), ("pad", 0), ("R", 1), ("N", 1), ("Ho", 19)):
        m = ok()
        setattr(m[1], field, value)
        assert run(m) == EINVAL, field
    for field in ("scale", "shift", "res"):                        # which optional pointers are NULL must agree
        m = ok()
        setattr(m[1], field, None if field == "shift" else 0x5000000)
        assert run(m) == EINVAL, field
    for field in ("y2", "colsum", "colsum_ws"):                    # training forms: single calls only
        m = ok()
        setattr(m[0], field, 0x6000000)
        assert run(m) == EINVAL, field
    m = ok()
    for a in m:
        a.out_mode, a.K = L.OUT_CONVT2X2, 64
    assert run(m) == EINVAL
    # overlapping outputs: the same slice twice; slices one channel short of disjoint; dense outputs whose byte ranges meet
    m = ok()
    m[1].y = m[0].y
    assert run(m) == EINVAL
    m = ok()
    m[1].y = m[0].y + 63 * 2 + 2 - 16                              # (16-byte aligned, 8 channels inside member 0's slice)
    assert run(m) == EINVAL
    d = [head_args(2, 20, 64, 64, k=3, y=0x4000000), head_args(2, 20, 64, 64, k=3, y=0x4000000 + 2 * 20 * 20 * 64 * 2 - 64)]
    assert run(d) == EINVAL
    d[1].y = 0x4000000 + 2 * 20 * 20 * 64 * 2                       # back to back: legal
    assert batch_choice(lib, d)[0] == 0
    m = ok()
    m[1].x += 2                                                    # per-member alignment rules
    assert run(m) == -2
    # a tile the batched kernels are not instantiated for
    m = [head_args(2, 20, 64, 96, k=1, hint=(96 << 16) | 64, y=0x4000000 + j * 0x100000) for j in range(2)]
    assert run(m) == EINVAL


def test_batch_choice_equals_single_choice_for_one_member(lib):
    """n = 1: the batch chooser is the single-call chooser, for every row of the variant table that is a legal member (plain NHWC output and a
    kernel the batched form instantiates); every other row is refused."""
    legal = 0
    for row in KR.VARIANTS:
        for dt in row.dtypes:
            a = KR.conv_args(L, row, dt)
            single = KR.kernel_choice(L, lib, a)
            rc, got = batch_choice(lib, [a])
            if row.convt or not in_batch_set(single):
                assert rc == EINVAL, (row.name, dt, single)
            else:
                assert rc == 0 and got == single, (row.name, dt, single, got)
                legal += 1
    assert legal >= 12


# rows 3, 4 / 6, 7, 8 of the merged-heads table at batch 16 x 640^2: (members, Cin, K, k, act, fp32 output) -> choice at 80^2 / 40^2 / 20^2.
# The two 256 -> 256 convs together: 3200 tiles of 128 x 128 at 80^2 (a large grid); 800 at 40^2 would be a second, mostly empty round on the
# 512 workgroup slots -> 128 x 64; at 20^2 400 tiles of 128 x 64 are one full round (a single call has 200 and takes 64 x 64).
HEAD_BATCHES = {
    "3x3 64->64 x3": (3, 64, 64, 3, L.ACT_SILU, False, ((1, 64, 256, 0), (0, 64, 64, 1), (0, 64, 64, 1))),
    "1x1 256->256 x2": (2, 256, 256, 1, L.ACT_SILU, False, ((0, 128, 128, 1), (0, 128, 64, 1), (0, 128, 64, 1))),
    "1x1 64->64 f32 x2": (2, 64, 64, 1, L.ACT_NONE, True, ((0, 64, 64, 1),) * 3),
    "1x1 256->2 f32 x2": (2, 256, 2, 1, L.ACT_NONE, True, ({L.BF16: (2, 2, 128, 0), L.F16: (2, 2, 128, 0), L.F32: (0, 32, 64, 1)},) * 3),
}


@pytest.mark.parametrize("name", sorted(HEAD_BATCHES))
@pytest.mark.parametrize("dtype", [L.BF16, L.F16, L.F32])
def test_batch_choice_of_the_head_shapes(lib, name, dtype):
    """The ONE kernel choice of each head batch (the tile rules count the workgroups of all members) is pinned and is a kernel the batched
    form instantiates."""
    n, Cin, K, k, act, f32, pins = HEAD_BATCHES[name]
    for H, pin in zip((80, 40, 20), pins):
        kw = dict(N=16, H=H, Cin=Cin, K=K, k=k, act=act, dtype=dtype)
        if f32:      # the two [N,h,w,no] fp32 maps, pitch 68: different buffers
            es = 4 if dtype == L.F32 else 2
            members = [head_args(x=0x100000 + j * Cin * es, ldx=n * Cin, y=0x4000000 + j * 0x4000000 + (0 if K == 64 else 256), ldy=68, out_dtype=L.F32, **kw)
                       for j in range(n)]
        else:
            members = slices(n, K, **kw)
        rc, got = batch_choice(lib, members)
        if isinstance(pin, dict):
            pin = pin[dtype]
        assert rc == 0 and got == pin, (name, H, got)
        assert in_batch_set(got)


def test_plan_conv_batch_dependencies():
    """engine.Plan.conv_batch: ONE launch that depends on the writers of every member's input and is a dependency of every member's readers;
    FLOPs / bytes are the members' sums; overlapping member outputs raise.  No launch is executed (CPU tensors)."""
    from multitask_bonetumor_yolo_amd.engine import Plan
    p = Plan(torch.device("cpu"))
    w = torch.zeros(64, 64, dtype=torch.bfloat16)
    sh = torch.zeros(64)
    a = p.new(1, 8, 8, 64, L.BF16)
    src = p.new(1, 8, 8, 128, L.BF16)
    dst = p.new(1, 8, 8, 128, L.BF16)
    p.conv(a, w, src.slice(0, 64), name="w0")                                   # 0
    p.conv(a, w, src.slice(64, 64), name="w1")                                  # 1
    p.conv_batch([(src.slice(0, 64), w, dst.slice(0, 64), sh), (src.slice(64, 64), w, dst.slice(64, 64), sh)], name="m0 + m1")   # 2
    r0, r1 = p.new(1, 8, 8, 64, L.BF16), p.new(1, 8, 8, 64, L.BF16)
    p.conv(dst.slice(0, 64), w, r0, name="r0")                                  # 3
    p.conv(dst.slice(64, 64), w, r1, name="r1")                                 # 4
    p.conv(a, w, src.slice(64, 64), name="war")                                 # 5: overwrites what the batch read
    assert len(p.launches) == 6 and p.launches[2].fn is p.lib.mtbt_conv2d_nhwc_batch
    assert p.dependencies() == [[], [], [0, 1], [2], [2], [1, 2]]
    one = p.launches[0]
    assert p.launches[2].flops == 2 * one.flops and p.launches[2].bytes == 2 * one.bytes and p.launches[2].name == "m0 + m1"
    with pytest.raises(ValueError, match="overlap"):
        p.conv_batch([(src.slice(0, 64), w, dst.slice(0, 64), sh), (src.slice(64, 64), w, dst.slice(32, 64), sh)])
    with pytest.raises(ValueError, match="overlap"):
        p.conv_batch([(src.slice(0, 64), w, r0, sh), (src.slice(64, 64), w, r0, sh)])
    with pytest.raises(ValueError):
        p.conv_batch([])
    assert len(p.launches) == 6
    # the per-call policy ORs its bits onto the plan's (default policy = bits 0-2)
    assert p.conv(a, w, r0, policy=32).policy == (0x100 | 7 | 32) and p.conv(a, w, r0).policy == 0


def test_plan_dwconv_multiplier_form():
    from multitask_bonetumor_yolo_amd.engine import Plan
    p = Plan(torch.device("cpu"))
    x, y = p.new(1, 8, 8, 256, L.BF16), p.new(1, 8, 8, 512, L.BF16)
    w, v = torch.zeros(9, 512, dtype=torch.bfloat16), torch.zeros(512)
    p.dwconv(x, w, y, 3, scale=v, shift=v, act=L.ACT_SILU, name="dw x2")
    assert p.launches[0].fn is p.lib.mtbt_dwconv3x3_mult_nhwc and p.launches[0].args[9:11] == (256, 2)


def test_merged_head_weight_packing():
    """Row 1 (the first 3x3 convs of cv2 / cv2 / cv4 as one conv) and rows 2 / 5 (depthwise filters side by side): the concatenated folded
    weights / scales / shifts equal the per-branch `_bn_fold` results slice by slice."""
    from multitask_bonetumor_yolo_amd import model as M
    torch.manual_seed(0)
    det, seg = M.Detect(nc=2, ch=(256,) * 3), M.Segment(nc=2, nm=32, npr=256, ch=(256,) * 3)
    for m in list(det.modules()) + list(seg.modules()):
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5), m.bias.data.normal_(), m.running_mean.normal_(), m.running_var.uniform_(0.5, 2.0)
    det.eval(), seg.eval()
    for i in range(3):
        blocks = [det.cv2[i][0], seg.cv2[i][0], seg.cv4[i][0]]
        w, sh = M.pack_convblocks(blocks)
        assert tuple(w.shape) == (192, 9 * 256) and tuple(sh.shape) == (192,)
        for j, b in enumerate(blocks):
            scale, shift = M._bn_fold(b.bn, b.conv.bias)
            assert torch.equal(w[64 * j:64 * (j + 1)], M._krsc(b.conv.weight).float() * scale[:, None])
            assert torch.equal(sh[64 * j:64 * (j + 1)], shift)
        for k in (0, 1):
            blocks = [det.cv3[i][k][0], seg.cv3[i][k][0]]
            w, sc, sh = M.pack_dwblocks(blocks)
            assert tuple(w.shape) == (9, 512) and w.is_contiguous()
            for j, b in enumerate(blocks):
                scale, shift = M._bn_fold(b.bn)
                assert torch.equal(w[:, 256 * j:256 * (j + 1)], b.conv.weight.detach().reshape(256, 9).t())
                assert torch.equal(sc[256 * j:256 * (j + 1)], scale) and torch.equal(sh[256 * j:256 * (j + 1)], shift)


def test_heads_merged_is_a_plan_option_and_not_an_autotune_knob(monkeypatch):
    from multitask_bonetumor_yolo_amd import graphed, model as M
    assert M.PLAN_OPTION_DEFAULTS["HEADS_MERGED"] == "0"
    assert "HEADS_MERGED" not in str(graphed.AUTOTUNE_KNOBS)
    m = torch.nn.Module()
    assert M.plan_option(m, "HEADS_MERGED") == "0"
    monkeypatch.setenv("MTBT_HEADS_MERGED", "1")
    assert M.plan_option(m, "HEADS_MERGED") == "1"
    m.plan_options = {"HEADS_MERGED": "0"}
    assert M.plan_option(m, "HEADS_MERGED") == "0"
