"""Kernel-level parity of the fp16 arithmetic mode (BASELINE configs[4]) against fp64 references, and exact-rounding tests of every store path.

Every comparison uses tests/kernel_reference.py: an fp64 CPU reference computed from the operands exactly as the kernel reads them, and a
per-element bound built from stated terms (one output rounding, fp32 accumulation, documented approximations).  The conv rows come from its
variant table; each row first asserts (mtbt_conv_kernel_choice, on the very arguments it launches with) that it reaches the kernel it names.

Exact-rounding tests use small-integer operands, a power-of-two scale and a dyadic shift: every product and partial sum is exact in fp32, so
the result does not depend on accumulation order and the kernel output must equal, bit for bit, the exact fp32 result rounded ONCE."""
import ctypes as C
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import kernel_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd.engine import Act, Plan

DEV = "cuda:0"
F16 = torch.float16
ROW_PARAMS = [(r, d) for r in R.VARIANTS for d in r.dtypes]
ROW_IDS = [f"{r.name}-{R.DNAME[d]}" for r, d in ROW_PARAMS]


def nhwc(t, dtype):  # [N,C,H,W] cpu -> dense NHWC cuda in the storage dtype
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def run(p):
    p.run()
    torch.cuda.synchronize()


def run_conv_row(row, dtype, x, w, scale, shift, res):
    """Launch one variant-table row: x / w / res in storage precision (NCHW, fp64), scale / shift fp32 (or None).  Returns the output as an
    NCHW fp64 tensor in the reference's layout (ConvT: the 4 * Cout packed rows), after checking the kernel choice and that nothing
    outside the output slice was written."""
    p = Plan(torch.device(DEV))
    p.conv_policy = row.policy
    K = row.K
    out_dt = torch.float32 if row.out == "f32" else dtype
    if row.convt:
        ybuf = torch.full((row.N, 2 * row.H, 2 * row.W, K // 4), 7.0, dtype=out_dt, device=DEV)
        ya = Act.of(ybuf)
    else:
        ybuf = torch.full((row.N, row.Ho, row.Wo, row.pitch), 7.0, dtype=out_dt, device=DEV)
        ya = Act.of(ybuf).slice(row.c0, K)
    wp = w.permute(0, 2, 3, 1).reshape(K, -1).contiguous().to(DEV, dtype)
    a = p.conv(Act.of(nhwc(x, dtype)), wp, ya, R=row.k, S=row.k, stride=row.stride, pad=row.pad,
               scale=scale.to(DEV) if scale is not None else None, shift=shift.to(DEV) if shift is not None else None, act=row.act,
               res=Act.of(nhwc(res, dtype)) if res is not None else None, out_mode=L.OUT_CONVT2X2 if row.convt else L.OUT_NHWC,
               tile_hint=row.hint)
    assert R.kernel_choice(L, p.lib, a) == row.expect, row.name
    run(p)
    y = ybuf.double().cpu()
    if row.convt:
        return y.view(row.N, row.H, 2, row.W, 2, K // 4).permute(0, 2, 4, 5, 1, 3).reshape(row.N, K, row.H, row.W)
    assert torch.all(y[..., :row.c0] == 7.0) and torch.all(y[..., row.c0 + K:] == 7.0), "written outside the output slice"
    return y[..., row.c0:row.c0 + K].permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. every row of the variant table, every dtype it runs in, against the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,dtype", ROW_PARAMS, ids=ROW_IDS)
def test_conv_variant_parity(row, dtype):
    g = torch.Generator().manual_seed(sum(map(ord, row.name)))
    x = R.storage(torch.randn(row.N, row.C, row.H, row.W, generator=g), dtype)
    w = R.storage(torch.randn(row.K, row.C, row.k, row.k, generator=g) / (row.C * row.k * row.k) ** 0.5, dtype)
    scale = torch.rand(row.K, generator=g) + 0.5 if row.scale else None
    shift = torch.randn(row.K, generator=g) * 0.1
    res = R.storage(torch.randn(row.N, row.K, row.Ho, row.Wo, generator=g), dtype) if row.res else None
    out_dt = torch.float32 if row.out == "f32" else dtype
    ref, bnd = R.conv_ref(x, w, row.stride, row.pad, scale, shift, row.act, res, out_dt)
    R.check(run_conv_row(row, dtype, x, w, scale, shift, res), ref, bnd, f"{row.name} {R.DNAME[dtype]}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. exact rounding: integer operands, power-of-two scale, dyadic shift
# ---------------------------------------------------------------------------------------------------------------------------------------
EXACT_ROWS = ["g128x128w", "g128x128n", "g96x128w", "g32x64n", "g64x64w_slice", "g128x64n_slice", "direct64", "direct128", "rowreuse64",
              "rowreuse128", "convt2x2", "pw_stream"]
EXACT_PARAMS = [(n, d) for n in EXACT_ROWS for d in R.ROWS[n].dtypes]


exact_operands, rounded_once = R.exact_operands, R.rounded_once     # shared with tests/test_gpu_conv_train_epilogue.py


@pytest.mark.parametrize("name,dtype", EXACT_PARAMS, ids=[f"{n}-{R.DNAME[d]}" for n, d in EXACT_PARAMS])
def test_conv_exact_rounding(name, dtype):
    """Vector epilogue (dense rows) and scalar epilogue (the slices at channel offset 2), implicit GEMM wide / narrow, both direct
    formulations, residual rows (a conv result rounded before the residual add would differ: double rounding), ConvT 2x2, the streaming
    head conv.  Activations are none: only the store rounds."""
    row = dataclasses.replace(R.ROWS[name], act=R.ACT_NONE)
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x, w, scale, shift, res, exact = exact_operands(row, dtype, g)
    out_dt = torch.float32 if row.out == "f32" else dtype
    want = rounded_once(exact, out_dt)
    got = run_conv_row(row, dtype, x, w, scale, shift, res)
    if out_dt != torch.float32:
        assert (want != exact).float().mean().item() > 0.3, "the test values must need rounding"
    diff = got != want
    assert not diff.any(), f"{int(diff.sum())} of {diff.numel()} outputs differ from the once-rounded exact result, e.g. got " \
                           f"{got[diff][:4].tolist()} want {want[diff][:4].tolist()} exact {exact[diff][:4].tolist()}"


@pytest.mark.parametrize("name", ["g128x128w", "g64x64w_slice", "direct128", "rowreuse128"])
def test_fp16_conv_store_saturates(name):
    """Accumulations past +-65504 are stored as exactly +-65504, never inf, through the conv epilogues (vector and scalar stores)."""
    row = dataclasses.replace(R.ROWS[name], act=R.ACT_NONE)
    g = torch.Generator().manual_seed(7)
    x, w, scale, shift, res, exact = exact_operands(row, F16, g, target=40000.0)
    got = run_conv_row(row, F16, x, w, scale, shift, res)
    assert (exact.abs() > 65520).sum().item() > 10, "the test must overflow the binary16 range"
    assert torch.isfinite(got).all()
    assert torch.equal(got, rounded_once(exact, F16))
    assert torch.equal(got[exact > 65504], torch.full_like(got[exact > 65504], 65504.0))


@pytest.mark.parametrize("name", ["g128x128w", "g64x64w_slice", "rowreuse64"])
def test_fp16_conv_store_keeps_subnormals(name):
    """A power-of-two scale that puts the outputs in the binary16 subnormal range: rounded to nearest even, not flushed to zero."""
    row = dataclasses.replace(R.ROWS[name], act=R.ACT_NONE, res=False)
    g = torch.Generator().manual_seed(8)
    x, w, scale, shift, res, exact = exact_operands(row, F16, g, scale_pow=-29, shift_step=0.0)
    want = rounded_once(exact, F16)
    sub = (want != 0) & (want.abs() < 2.0 ** -14)
    assert sub.float().mean().item() > 0.5 and (want != exact).float().mean().item() > 0.5
    got = run_conv_row(row, F16, x, w, scale, shift, None)
    assert torch.equal(got, want), f"{int((got != want).sum())} subnormal outputs differ"


def test_dwconv_affine_exact_rounding():
    """Depthwise 7x7, scale / shift form, act none: integer operands, power-of-two scale, dyadic shift -> the once-rounded exact result."""
    g = torch.Generator().manual_seed(9)
    N, Cc, H, W = 2, 384, 12, 20
    x = torch.randint(-8, 9, (N, Cc, H, W), generator=g).double()
    w = torch.randint(-8, 9, (Cc, 1, 7, 7), generator=g).double()
    sc = (2.0 ** (4 + torch.randint(0, 2, (Cc,), generator=g))).float()
    sh = torch.randint(-64, 65, (Cc,), generator=g).float() * 0.25
    exact = F.conv2d(x, w, None, 1, 3, groups=Cc) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    assert torch.equal(exact.float().double(), exact)
    for dtype in R.DTYPES:
        p = Plan(torch.device(DEV))
        ya = Act.of(torch.zeros(N, H, W, Cc, dtype=dtype, device=DEV))
        p.dwconv(Act.of(nhwc(x, dtype)), w.reshape(Cc, 49).t().contiguous().to(DEV, dtype), ya, 7, scale=sc.to(DEV), shift=sh.to(DEV), act=0)
        run(p)
        got = ya.buf.double().cpu().permute(0, 3, 1, 2)
        want = rounded_once(exact, dtype)
        assert torch.equal(got, want), (R.DNAME[dtype], int((got != want).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the other fp16 kernels against fp64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 96, 9, 11), (1, 192, 8, 8), (1, 768, 5, 6), (1, 384, 4, 4), (1, 96, 20, 37), (2, 384, 17, 16),
                                   (1, 384, 40, 40), (2, 384, 12, 20), (1, 768, 20, 24), (1, 192, 16, 32)])
def test_fp16_dwconv7_layernorm(shape):
    """ConvNeXt conv_dw + norm in one kernel (the shapes of test_dwconv7_layernorm: ragged, half-width and full tiles)."""
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(6)
    x = R.storage(torch.randn(N, Cc, H, W, generator=g), F16)
    w = R.storage(torch.randn(Cc, 1, 7, 7, generator=g) / 7, F16)
    b = torch.randn(Cc, generator=g) * 0.1
    lw, lb = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    v = (F.conv2d(x, w, None, 1, 3, groups=Cc) + b.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1).reshape(-1, Cc)
    verr = (R.ACC * F.conv2d(x.abs(), w.abs(), None, 1, 3, groups=Cc) + R.EPI * b.double().abs().view(1, -1, 1, 1))
    verr = verr.permute(0, 2, 3, 1).reshape(-1, Cc).amax(-1, keepdim=True)
    ref = F.layer_norm(v, (Cc,), lw.double(), lb.double(), 1e-6)
    bnd = R.ln_bound(ref, v, lw, lb, 1e-6, verr, F16)
    p = Plan(torch.device(DEV))
    ya = Act.of(torch.zeros(N, H, W, Cc, dtype=F16, device=DEV))
    p.dwconv(Act.of(nhwc(x, F16)), w.reshape(Cc, 49).t().contiguous().to(DEV, F16), ya, 7, bias=b.to(DEV), lnw=lw.to(DEV), lnb=lb.to(DEV), eps=1e-6)
    run(p)
    R.check(ya.buf.double().cpu().reshape(-1, Cc), ref, bnd, f"dwconv7+LN {shape}")


def _dw_affine(N, Cc, H, W, ks, act, seed):
    g = torch.Generator().manual_seed(seed)
    x = R.storage(torch.randn(N, Cc, H, W, generator=g), F16)
    w = R.storage(torch.randn(Cc, 1, ks, ks, generator=g) / ks, F16)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    ref, bnd = R.conv_ref(x, w, 1, ks // 2, sc, sh, act, None, F16, groups=Cc)
    p = Plan(torch.device(DEV))
    ya = Act.of(torch.zeros(N, H, W, Cc, dtype=F16, device=DEV))
    p.dwconv(Act.of(nhwc(x, F16)), w.reshape(Cc, ks * ks).t().contiguous().to(DEV, F16), ya, ks, scale=sc.to(DEV), shift=sh.to(DEV), act=act)
    run(p)
    R.check(ya.buf.double().cpu().permute(0, 3, 1, 2), ref, bnd, f"dwconv{ks} act {act} {(N, Cc, H, W)}")


def test_fp16_dwconv3_affine_silu():
    _dw_affine(2, 256, 7, 10, 3, R.ACT_SILU, 7)


@pytest.mark.parametrize("shape", [(2, 384, 12, 20), (1, 768, 8, 24), (1, 192, 16, 16), (2, 96, 9, 11), (1, 256, 40, 40)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_fp16_dwconv7_affine(shape, act):
    _dw_affine(*shape, 7, act, 9)


@pytest.mark.parametrize("Cc,offset", [(96, 0.5), (192, 0.5), (768, 0.5), (96, 1000.0), (768, 1000.0)])
def test_fp16_layernorm(Cc, offset):
    """offset 1000 with unit spread pins the two-pass variance: E[x^2] - mean^2 in fp32 would be off by percent."""
    g = torch.Generator().manual_seed(8)
    x = R.storage(torch.randn(2, 5, 7, Cc, generator=g) * (2.0 if offset < 1 else 1.0) + offset, F16).reshape(-1, Cc)
    lw, lb = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    ref = F.layer_norm(x, (Cc,), lw.double(), lb.double(), 1e-6)
    bnd = R.ln_bound(ref, x, lw, lb, 1e-6, 0.0, F16)
    p = Plan(torch.device(DEV))
    ya = Act.of(torch.zeros(2, 5, 7, Cc, dtype=F16, device=DEV))
    p.layernorm(Act.of(x.reshape(2, 5, 7, Cc).to(DEV, F16)), lw.to(DEV), lb.to(DEV), 1e-6, ya)
    run(p)
    R.check(ya.buf.double().cpu().reshape(-1, Cc), ref, bnd, f"layernorm C={Cc} offset={offset}")


def test_fp16_bifpn_fuse_modes():
    """Weighted sum with every resample mode (identity, bilinear x2, 2x2 mean, nearest x2, 2x2 max) and the WeightedAdd bug form
    (sum of w_i + f_i): fp32 arithmetic of at most ~8 operations per term (2^-20 of the summed magnitudes) and one fp16 rounding."""
    g = torch.Generator().manual_seed(9)
    Cc = 64
    mid, small, big = (R.storage(torch.randn(2, Cc, h, w, generator=g), F16) for h, w in ((8, 6), (4, 3), (16, 12)))
    rs = {0: lambda t: t, 1: lambda t: F.interpolate(t, scale_factor=2, mode="bilinear"), 2: lambda t: F.avg_pool2d(t, 2),
          3: lambda t: F.interpolate(t, scale_factor=2, mode="nearest"), 4: lambda t: F.max_pool2d(t, 2)}
    wts = [0.3, 0.45, 0.25]
    cases = [([mid, small], [0, 1], False), ([mid, mid, big], [0, 0, 2], False), ([mid, small], [0, 3], False), ([mid, big], [0, 4], False),
             ([mid, small], [0, 3], True), ([mid, small, big], [0, 1, 2], False)]
    for ins, modes, bug in cases:
        parts = [rs[m](t) for t, m in zip(ins, modes)]
        mags = [rs[m](t.abs()) if m != 4 else rs[m](t).abs() for t, m in zip(ins, modes)]
        if bug:
            ref = sum(wv + t for wv, t in zip(wts, parts))
            mag = sum(abs(wv) + t for wv, t in zip(wts, mags))
        else:
            ref = sum(wv * t for wv, t in zip(wts, parts))
            mag = sum(abs(wv) * t for wv, t in zip(wts, mags))
        bnd = R.output_rounding(ref, F16) + 2.0 ** -20 * mag
        p = Plan(torch.device(DEV))
        ya = Act.of(torch.zeros(2, 8, 6, Cc, dtype=F16, device=DEV))
        p.fuse([Act.of(nhwc(t, F16)) for t in ins], wts[:len(ins)], modes, ya, bug=bug)
        run(p)
        R.check(ya.buf.double().cpu().permute(0, 3, 1, 2), ref, bnd, f"fuse {modes} bug={bug}")


@pytest.mark.parametrize("shape", [(3, 256, 5, 4), (2, 768, 7, 9)])
def test_fp16_gap_fc(shape):
    """Global average pool of fp16 input, then Linear in fp32 (fp32 output): sums of HW and C terms, (HW + C/64 + 16) 2^-24 of sum |w| mean |x|."""
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(10)
    x = R.storage(torch.randn(N, Cc, H, W, generator=g), F16)
    w, b = torch.randn(2, Cc, generator=g) / 16, torch.randn(2, generator=g)
    ref = F.linear(x.mean((2, 3)), w.double(), b.double())
    bnd = (H * W + Cc / 64 + 16) * 2.0 ** -24 * (x.abs().mean((2, 3)) @ w.double().abs().t() + b.double().abs()) + R.output_rounding(ref, torch.float32)
    p = Plan(torch.device(DEV))
    y = torch.zeros(N, 2, device=DEV)
    p.gap_fc(Act.of(nhwc(x, F16)), w.to(DEV), b.to(DEV), y)
    run(p)
    R.check(y.double().cpu(), ref, bnd, "gap_fc")


@pytest.mark.parametrize("path,W", [("mfma", 128), ("generic", 40)])
def test_fp16_stem(path, W):
    """ConvNeXt stem (4x4/4 conv + LayerNorm2d), fp32 image and weights.  The MFMA kernel (Cout 96, (W / 4) % 16 == 0) converts the image
    and the weights to fp16 MFMA operands (pointwise.hip pk16 / StemCvt): the reference rounds them the same way.  The generic kernel
    computes in fp32 from the fp32 operands: the reference does not round them."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 32, W, generator=g)
    w = torch.randn(96, 3, 4, 4, generator=g) / 7
    b = torch.randn(96, generator=g) * 0.1
    lw, lb = torch.rand(96, generator=g) + 0.5, torch.randn(96, generator=g) * 0.1
    xr, wr = (R.storage(x, F16), R.storage(w, F16)) if path == "mfma" else (x.double(), w.double())
    v = (F.conv2d(xr, wr, b.double(), 4)).permute(0, 2, 3, 1).reshape(-1, 96)
    verr = (R.ACC * F.conv2d(xr.abs(), wr.abs(), None, 4) + R.EPI * b.double().abs().view(1, -1, 1, 1)).permute(0, 2, 3, 1).reshape(-1, 96)
    ref = F.layer_norm(v, (96,), lw.double(), lb.double(), 1e-6)
    bnd = R.ln_bound(ref, v, lw, lb, 1e-6, verr.amax(-1, keepdim=True), F16)
    p = Plan(torch.device(DEV))
    ya = Act.of(torch.zeros(2, 8, W // 4, 96, dtype=F16, device=DEV))
    p.stem(x.to(DEV), w.reshape(96, 48).contiguous().to(DEV), b.to(DEV), lw.to(DEV), lb.to(DEV), 1e-6, ya)
    run(p)
    R.check(ya.buf.double().cpu().reshape(-1, 96), ref, bnd, f"stem {path}")


def _fp16_spacing_below(h16):
    """Distance from |h| (an fp16 value, fp64 tensor) down to the next smaller fp16 magnitude (2^-24 at zero)."""
    a = h16.abs().to(F16)
    prev = (a.view(torch.int16) - 1).clamp(min=0).view(F16).double()
    return torch.where(a == 0, torch.full_like(h16, 2.0 ** -24), a.double() - prev)


@pytest.mark.parametrize("D,M", [(96, 1024), (96, 1000), (192, 512), (192, 517), (384, 384), (384, 128 * 7 + 37)])
def test_fp16_convnext_mlp_fused(D, M):
    """mtbt_convnext_mlp_fused_dt(MTBT_F16): y = res + W2' h + b2', h = fp16(gelu_poly(W1 t + b1)) -- the kernel stores GELU(hidden) as
    fp16 (mlp_fused.hip pk2<f16_t>) and feeds it to the second MFMA, so the reference rounds h there too.  The reference evaluates the
    kernel's own polynomial GELU in fp64 (kernel_reference.gelu_poly64) instead of erf + 2.3e-4: a fixed 2.3e-4 on each of the 4D hidden
    units, summed through W2, would be looser than the hidden rounding it has to see.  The fp32 accumulation of fc1 can move a hidden value
    that lies near an fp16 rounding midpoint to the other neighbour: those units (flagged from the fc1 accumulation bound) may be off by one
    fp16 spacing, weighted by |W2|.  Rows past M are not written."""
    from multitask_bonetumor_yolo_amd.model import _permute_hidden
    g = torch.Generator().manual_seed(D + M)
    t = R.storage(torch.randn(M, D, generator=g), F16)
    res = R.storage(torch.randn(M, D, generator=g) * 0.1, F16)
    w1 = R.storage(torch.randn(4 * D, D, generator=g) / D ** 0.5, F16)
    w2 = R.storage(torch.randn(D, 4 * D, generator=g) / (4 * D) ** 0.5, F16)
    b1, b2 = torch.randn(4 * D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1
    pre = t @ w1.t() + b1.double()
    pre_err = R.ACC * (t.abs() @ w1.abs().t() + b1.double().abs())
    h64 = R.gelu_poly64(pre)
    h16 = h64.to(F16).double()
    below = _fp16_spacing_below(h16)
    above = _fp16_spacing_below(h16.abs().to(F16).view(torch.int16).add(1).view(F16).double())
    delta = R.ACT_LIPSCHITZ[R.ACT_GELU_POLY] * pre_err + 2.0 ** -21 * (1 + h64.abs())     # fc1 accumulation + fp32 polynomial
    flip = (h64 - h16).abs() >= 0.5 * torch.minimum(below, above) - delta
    ref = res + h16 @ w2.t() + b2.double()
    bnd = (R.output_rounding(ref, F16) + R.ACC * (h16.abs() @ w2.abs().t() + res.abs() + b2.double().abs())
           + (flip.double() * torch.maximum(below, above)) @ w2.abs().t())
    extra = 3
    y = torch.full((M + extra, D), 7.0, dtype=F16, device=DEV)
    dev = [v.to(DEV) for v in (t.half(), res.half(), w1.half(), b1, _permute_hidden(w2.half()).contiguous(), b2)]
    lib = L.load()
    rc = lib.mtbt_convnext_mlp_fused_dt(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(),
                                        dev[5].data_ptr(), y.data_ptr(), M, D, L.F16, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = y.double().cpu()
    assert torch.all(got[M:] == 7.0), "written past row M"
    assert flip.double().mean().item() < 0.2
    R.check(got[:M], ref, bnd, f"mlp D={D} M={M}")


def test_fp16_cast_round_trip():
    """mtbt_cast f32 -> f16 rounds to nearest even (ties, subnormals, values just below the saturation limit) and saturates at +-65504;
    f16 -> f32 is exact; every finite fp16 value survives f16 -> f32 -> f16 bit for bit."""
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cast(src, sd, dd, out_dtype):
        dst = torch.empty(src.numel(), dtype=out_dtype, device=DEV)
        L.check(lib.mtbt_cast(src.data_ptr(), dst.data_ptr(), src.numel(), sd, dd, stream), "cast")
        torch.cuda.synchronize()
        return dst.cpu()

    g = torch.Generator().manual_seed(11)
    ties = torch.tensor([1 + 2 ** -11, 1 + 3 * 2 ** -11, 2048 + 1, 2048 + 3, 2 ** -24 * 0.5, 2 ** -24 * 1.5, 2 ** -24 * 2.5, 65504 + 8, 65504 + 15.99,
                         65520.0, 6.1e-5, 5.9e-5], dtype=torch.float32)
    src = torch.cat([ties, -ties, torch.randn(4096, generator=g) * 1000, torch.randn(4096, generator=g) * 1e-5,
                     torch.randn(1024, generator=g) * 1e5]).contiguous()
    got = cast(src.to(DEV), L.F32, L.F16, F16)
    want = src.clamp(-65504, 65504).half()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got != want).sum())
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(F16)
    fin = bits[torch.isfinite(bits)].contiguous()
    f32 = cast(fin.to(DEV), L.F16, L.F32, torch.float32)
    assert torch.equal(f32, fin.float())
    back = cast(f32.to(DEV), L.F32, L.F16, F16)
    assert torch.equal(back.view(torch.int16), fin.view(torch.int16))
