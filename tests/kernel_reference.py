"""Shared fp64 references, per-element error bounds and the conv variant table of the kernel-level tests.

A plain module (no fixtures): tests/test_cpu_kernel_reference.py checks it on the CPU, tests/test_gpu_fp16.py runs it on the GPU.

References are computed in fp64 on the CPU from the operands exactly as the kernel sees them: activations, weights and residuals rounded to
the storage dtype (`storage`), scale / shift / bias kept in fp32.  Where a kernel rounds an intermediate, the reference rounds it at the same
point and says so.

Bounds are per element and built from stated terms, never from one "relative to the maximum" constant:
  * one rounding of the output to its storage type: 2^-11 |ref| (fp16, plus half the smallest subnormal), 2^-8 |ref| (bf16), 2^-24 |ref| (fp32);
  * fp32 accumulation: ACC * sum |x * w| (ACC = 2^-22: the order 2^-23 of an fp32 sum, with a factor 2 for the products of the fp32 mode);
  * fp32 epilogue arithmetic (affine, residual add): 2^-23 of the magnitude of its operands;
  * the activation's fp32 evaluation with the hardware exp2 / rcp (common.h act_apply): 2^-20 (1 + |v|);
  * a fixed term only where an approximation is documented: the polynomial GELU (ACT_GELU_POLY, common.h gelu_poly) has |err| <= 2.3e-4,
    the Abramowitz-Stegun erf of ACT_DGELU (common.h fast_erf) has |err| <= 1.5e-7;
  * the polynomial GELU derivative (ACT_DGELU_POLY, common.h gelu_poly_grad): 2^-23 of the absolute terms of its Horner chain
    (gelu_poly_grad_condition), which cancel to a small result near |z| = 4.

The training face of the conv kernels (second output y2, the derivative epilogues MTBT_ACT_D*, a residual that IS the output) has its own
references (preact_ref, deriv_ref, act_grad64) and its own table, TRAIN_VARIANTS; tests/test_gpu_conv_train_epilogue.py runs it.

The depthwise kernels (LayerNorm form, scale / shift form, training outputs, depth multiplier) have the table DW_VARIANTS and the references
dw_sums / dw_ln_ref / dw_row_reference; tests/test_gpu_dwconv_variants.py runs it.  They add no term to the list above: the scale / shift
form is affine_act_ref on the depthwise sums, the LayerNorm form ln_bound with an input error of ACC * sum |x * w| + EPI * |bias|, and the
LayerNorm input kept for training (raw) preact_ref with the bias as the shift: conv + bias rounded once.

The fused inference kernels (ConvT 2x2 -> conv 3x3 as one direct conv, the BiFPN node, the ConvNeXt MLP) have the tables UPCONV_VARIANTS,
NODE_VARIANTS and MLP_VARIANTS and the references upconv_ref / node_ref / mlp_ref; tests/test_gpu_fused_variants.py runs them.  They add no
term either; an intermediate that a kernel rounds to the storage type is rounded at the same point (round_flips).
"""
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

# activation codes of include/mtbt_hip.h (MTBT_ACT_*)
ACT_NONE, ACT_SILU, ACT_ELU, ACT_GELU, ACT_GELU_POLY = 0, 1, 2, 3, 4
ACT_DSILU, ACT_DELU, ACT_DGELU, ACT_DGELU_POLY = 5, 6, 7, 8       # y = affine * act'(res): the backward epilogues
GELU_POLY_ERR = 2.3e-4
ERF_AS_ERR = 1.5e-7              # common.h fast_erf: Abramowitz-Stegun 7.1.26
ACC = 2.0 ** -22
EPI = 2.0 ** -23
ACT_EVAL = 2.0 ** -20
ACT_LIPSCHITZ = {ACT_NONE: 1.0, ACT_SILU: 1.1, ACT_ELU: 1.0, ACT_GELU: 1.13, ACT_GELU_POLY: 1.13}

DTYPES = (torch.float16, torch.bfloat16, torch.float32)
DNAME = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}


def storage(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """t as the kernel reads it from a `dtype` buffer, in fp64."""
    return t.to(dtype).double()


def output_rounding(ref: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """One round-to-nearest of the exact result into `out_dtype`."""
    a = ref.abs()
    if out_dtype == torch.float16:
        return a * 2.0 ** -11 + 2.0 ** -25
    if out_dtype == torch.bfloat16:
        return a * 2.0 ** -8
    return a * 2.0 ** -24


# the fp32 coefficients of P in common.h gelu_poly, highest power of s = xc^2 first
GELU_POLY_C = [float(torch.tensor(v, dtype=torch.float32)) for v in
               (2.1609857e-08, -1.5335673e-06, 4.6542096e-05, -7.9887325e-04, 8.6900834e-03, -6.4366050e-02, 3.9770728e-01)]


def gelu_poly64(x: torch.Tensor) -> torch.Tensor:
    """common.h gelu_poly in fp64, from the same fp32 coefficients: x * (1/2 + xc P(xc^2)), xc = clamp(x, -4, 4)."""
    c = GELU_POLY_C
    xc = x.clamp(-4.0, 4.0)
    s = xc * xc
    p = torch.full_like(s, c[0])
    for ci in c[1:]:
        p = p * s + ci
    return x * (xc * p + 0.5)


def act64(v: torch.Tensor, act: int) -> torch.Tensor:
    """The exact activation (ACT_GELU_POLY: the erf GELU it approximates; see GELU_POLY_ERR)."""
    if act == ACT_NONE:
        return v
    if act == ACT_SILU:
        return F.silu(v)
    if act == ACT_ELU:
        return F.elu(v)
    if act in (ACT_GELU, ACT_GELU_POLY):
        return F.gelu(v)
    raise ValueError(act)


def act_error(pre: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_NONE:
        return torch.zeros_like(pre)
    e = ACT_EVAL * (1.0 + pre.abs())
    return e + GELU_POLY_ERR if act == ACT_GELU_POLY else e


def affine_act_ref(acc: torch.Tensor, mag: torch.Tensor, scale, shift, act: int, res: Optional[torch.Tensor], out_dtype):
    """Epilogue of the conv kernels (conv_epilogue.h): y = act(acc * scale + shift) + res, rounded once.  acc / mag: the fp64 sums
    sum x*w / sum |x*w| as [N, K, ...]; scale / shift fp32 per channel (None = 1 / 0); res already in storage precision.
    Returns (ref, bound)."""
    shp = (1, -1) + (1,) * (acc.dim() - 2)
    sc = scale.double().view(shp) if scale is not None else torch.ones(1, dtype=torch.float64)
    sh = shift.double().view(shp) if shift is not None else torch.zeros(1, dtype=torch.float64)
    pre = acc * sc + sh
    y = act64(pre, act)
    bnd = ACT_LIPSCHITZ[act] * (ACC * sc.abs() * mag + EPI * (pre.abs() + sh.abs())) + act_error(pre, act) + EPI * y.abs()
    if res is not None:
        y = y + res
        bnd = bnd + EPI * res.abs()
    return y, bnd + output_rounding(y, out_dtype)


def act_grad64(z: torch.Tensor, act: int) -> torch.Tensor:
    """act'(z) in fp64 (common.h act_grad; the D* codes and their forward codes mean the same derivative).  SiLU', ELU' and the erf GELU'
    in closed form.  ACT_DGELU_POLY: the derivative of gelu_poly64 by autograd on the fp64 forward polynomial (the kernel's gelu_poly_grad
    claims to be the exact derivative of what the forward computed, clamp region included), so no derivative coefficient is typed here.
    At |z| == 4 exactly the forward has a kink (autograd takes the inner side, the kernel the outer): the reference refuses such a z."""
    if act in (ACT_SILU, ACT_DSILU):
        s = torch.sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    if act in (ACT_ELU, ACT_DELU):
        return torch.where(z > 0, torch.ones_like(z), torch.exp(z))
    if act in (ACT_GELU, ACT_DGELU):
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act in (ACT_GELU_POLY, ACT_DGELU_POLY):
        assert not (z.abs() == 4.0).any(), "gelu_poly is not differentiable at |z| == 4"
        with torch.enable_grad():
            zz = z.detach().clone().requires_grad_()
            (g,) = torch.autograd.grad(gelu_poly64(zz).sum(), zz)
        return g.detach()
    raise ValueError(act)


def act_grad_error(z: torch.Tensor, act: int) -> torch.Tensor:
    """fp32 evaluation error of act'(z) with the hardware exp2 / rcp, like act_error; ACT_DGELU adds the one fixed term: its Phi(z) =
    (1 + erf) / 2 uses the Abramowitz-Stegun erf (common.h fast_erf, |error| <= 1.5e-7).  ACT_DGELU_POLY adds the conditioning of its
    Horner chain (gelu_poly_grad_condition): without it a faithful fp32 evaluation of the kernel's own formula misses the bound near
    |z| = 4 (tests/test_cpu_kernel_reference.py shows both)."""
    e = ACT_EVAL * (1.0 + z.abs())
    if act == ACT_DGELU_POLY:
        e = e + 2.0 ** -23 * gelu_poly_grad_condition(z)
    return e + 0.5 * ERF_AS_ERR if act == ACT_DGELU else e


def gelu_poly_grad_condition(z: torch.Tensor) -> torch.Tensor:
    """The magnitude the fp32 roundings of common.h gelu_poly_grad act on.  Inside |z| < 4 it returns fmaf(2 xc, Q(s), 1/2) with Q(s) =
    sum_j (j + 1) c_j s^j evaluated by Horner in fp32: the coefficient products (j + 1) c_j, s = xc * xc and each of the six FMAs round
    once, each on the scale of the ABSOLUTE terms sum_j (j + 1) |c_j| s^j -- which alternate in sign and reach 15 at s = 16, where Q itself
    is 0.08.  So the error is of the order 2^-24 |2 xc| sum_j (j + 1) |c_j| s^j (taken as 2^-23, like ACC), not of the order of the result:
    near |z| = 4 that is 4e-5, ten times ACT_EVAL (1 + |z|).  Outside, fmaf(xc, P16, 1/2) with the constant P16 = P(16) folded in fp32:
    |xc| sum_j |c_j| 16^j.  The weights (j + 1) come from differentiating the forward polynomial, its coefficients from GELU_POLY_C."""
    xc = z.clamp(-4.0, 4.0)
    s = xc * xc
    n = len(GELU_POLY_C)
    inside = sum((n - i) * abs(c) * s ** (n - 1 - i) for i, c in enumerate(GELU_POLY_C)) * (2.0 * xc).abs()
    outside = sum(abs(c) * 16.0 ** (n - 1 - i) for i, c in enumerate(GELU_POLY_C)) * xc.abs()
    return torch.where(z.abs() < 4.0, inside, outside)


def _affine(acc, scale, shift):
    shp = (1, -1) + (1,) * (acc.dim() - 2)
    sc = scale.double().view(shp) if scale is not None else torch.ones(1, dtype=torch.float64)
    sh = shift.double().view(shp) if shift is not None else torch.zeros(1, dtype=torch.float64)
    return sc, sh, acc * sc + sh


def deriv_ref(acc: torch.Tensor, mag: torch.Tensor, scale, shift, act: int, z: torch.Tensor, out_dtype):
    """The backward epilogues MTBT_ACT_D* (conv_epilogue.h MODE 2): y = (acc * scale + shift) * act'(z), rounded once; z is the residual
    operand in storage precision, so it is exact.  Bound: the affine's error through |act'(z)|, the derivative's fp32 evaluation error
    times |pre|, the product's rounding and the output rounding.  Returns (ref, bound)."""
    sc, sh, pre = _affine(acc, scale, shift)
    d = act_grad64(z, act)
    ref = pre * d
    bnd = d.abs() * (ACC * sc.abs() * mag + EPI * (pre.abs() + sh.abs())) + pre.abs() * act_grad_error(z, act) + EPI * ref.abs()
    return ref, bnd + output_rounding(ref, out_dtype)


def preact_ref(acc: torch.Tensor, mag: torch.Tensor, scale, shift, out_dtype):
    """The second output y2 of the training forward (conv_epilogue.h MODE 1): the pre-activation acc * scale + shift rounded once."""
    sc, sh, pre = _affine(acc, scale, shift)
    return pre, ACC * sc.abs() * mag + EPI * (pre.abs() + sh.abs()) + output_rounding(pre, out_dtype)


def conv_sums(x, w, stride, pad):
    """(sum x*w, sum |x*w|) of an NCHW fp64 conv: what the epilogue references start from."""
    return F.conv2d(x, w, None, stride, pad), F.conv2d(x.abs(), w.abs(), None, stride, pad)


def conv_ref(x, w, stride, pad, scale, shift, act, res, out_dtype, groups=1):
    """NCHW fp64 conv of storage-precision operands + the conv epilogue.  Returns (ref, bound)."""
    acc = F.conv2d(x, w, None, stride, pad, groups=groups)
    mag = F.conv2d(x.abs(), w.abs(), None, stride, pad, groups=groups)
    return affine_act_ref(acc, mag, scale, shift, act, res, out_dtype)


def ln_bound(y: torch.Tensor, v: torch.Tensor, g, b, eps: float, v_err, out_dtype) -> torch.Tensor:
    """Bound of a LayerNorm over the last dim of v (fp64 reference input, [P, C]) whose inputs carry an absolute error v_err ([P, 1]
    or scalar): fp32 sums of C terms (at most 16 sequential per lane, then a log2 tree: (log2 C + 16) 2^-24 of sum |v|) in the two
    passes, rsqrt to 2^-22, the affine in fp32 and one output rounding."""
    C = v.shape[-1]
    gam = (math.log2(C) + 16) * 2.0 ** -24
    mean = v.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (v - mean) * rstd
    dd = gam * v.abs().mean(-1, keepdim=True) + 2 * v_err            # error of x - mean
    dx = rstd * dd + xhat.abs() * (gam + 2.0 ** -21 + rstd * dd)      # error of xhat: the difference and rstd
    g, b = g.double(), b.double()
    return output_rounding(y, out_dtype) + g.abs() * dx + EPI * ((xhat * g).abs() + b.abs())


def check(out: torch.Tensor, ref: torch.Tensor, bnd: torch.Tensor, what: str = "") -> None:
    """Every element within its bound (NaN fails)."""
    out = out.double()
    err = (out - ref).abs()
    bad = ~(err <= bnd)
    if bad.any():
        ratio = torch.where(bad, err / bnd, torch.zeros_like(err))
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat index {i}: "
                             f"got {out.flatten()[i].item()!r}, ref {ref.flatten()[i].item()!r}, bound {bnd.flatten()[i].item():.3g}")


def within(out, ref, bnd) -> bool:
    try:
        check(out, ref, bnd)
        return True
    except AssertionError:
        return False


# ------------------------------------------------------------------------------------------------------------------------------------
# Conv variant table.  Each row: shape, act, residual, output (same dtype / fp32 / a channel slice at offset 2 of a K + 2 wide buffer:
# misaligned, so the scalar epilogue), tile hint / policy, and the mtbt_conv_kernel_choice tuple it must reach for every dtype:
# (kind 0 implicit GEMM / 1 direct 3x3 / 2 streaming head conv, channel tile, pixel tile, 128-byte K-steps (GEMM) / first formulation (direct)).
# Hint bits: (TC << 16) | TP; bit 27 = 64-byte (narrow) K-steps; bit 25 = the row-reuse direct kernel.  Policy bit 4 (0x100 | 7 | 16) selects
# the first direct formulation.  Every C is a multiple of 64, so the wide K-step (C % (128 / element size) == 0) is possible for every dtype.
# ------------------------------------------------------------------------------------------------------------------------------------
NARROW, ROW_REUSE = 1 << 27, 1 << 25
DIRECT_FIRST = 0x100 | 7 | 16


def hint(tc, tp, narrow=False):
    return (tc << 16) | tp | (NARROW if narrow else 0)


@dataclass(frozen=True)
class Row:
    name: str
    N: int
    H: int
    W: int
    C: int
    K: int
    k: int
    stride: int
    pad: int
    act: int
    res: bool
    out: str                 # "same" | "f32" | "slice"
    hint: int
    policy: int
    expect: Tuple[int, int, int, int]
    scale: bool = True
    convt: bool = False
    dtypes: Tuple[torch.dtype, ...] = field(default=DTYPES)

    @property
    def Ho(self):
        return (self.H + 2 * self.pad - self.k) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * self.pad - self.k) // self.stride + 1

    @property
    def pitch(self):
        return self.K + 2 if self.out == "slice" else self.K

    @property
    def c0(self):
        return 2 if self.out == "slice" else 0


S, E, G, GP = ACT_SILU, ACT_ELU, ACT_GELU, ACT_GELU_POLY
VARIANTS = [
    # implicit GEMM: every (TC, TP) tile with wide and narrow K-steps
    Row("g128x128w", 2, 9, 7, 64, 128, 3, 1, 1, S, False, "same", hint(128, 128), 0, (0, 128, 128, 1)),         # ragged M = 126
    Row("g128x128n", 1, 10, 10, 128, 160, 1, 1, 0, G, False, "same", hint(128, 128, True), 0, (0, 128, 128, 0)),  # K tail: 160 on TC 128
    Row("g128x64w", 2, 8, 8, 128, 128, 2, 2, 0, ACT_NONE, False, "same", hint(128, 64), 0, (0, 128, 64, 1)),      # 2x2 / 2 downsample
    Row("g128x64n", 1, 9, 11, 64, 128, 3, 1, 1, E, True, "same", hint(128, 64, True), 0, (0, 128, 64, 0)),        # residual
    Row("g96x128w", 2, 9, 7, 128, 96, 1, 1, 0, GP, True, "same", hint(96, 128), 0, (0, 96, 128, 1)),             # fc2-like + residual
    Row("g96x128n", 1, 12, 12, 64, 192, 3, 1, 1, S, False, "same", hint(96, 128, True), 0, (0, 96, 128, 0)),
    Row("g96x64w", 1, 7, 9, 64, 96, 3, 1, 1, E, False, "f32", hint(96, 64), 0, (0, 96, 64, 1)),                  # fp32 output
    Row("g96x64n", 2, 6, 6, 192, 96, 1, 1, 0, ACT_NONE, True, "same", hint(96, 64, True), 0, (0, 96, 64, 0)),
    Row("g64x128w", 1, 16, 10, 64, 48, 3, 1, 1, S, False, "same", hint(64, 128), 0, (0, 64, 128, 1)),           # K tail: 48 on TC 64
    Row("g64x128n", 2, 5, 13, 128, 64, 1, 1, 0, GP, False, "same", hint(64, 128, True), 0, (0, 64, 128, 0)),
    Row("g64x64w", 1, 10, 10, 64, 64, 3, 2, 1, S, False, "same", hint(64, 64), 0, (0, 64, 64, 1)),              # 3x3 / 2
    Row("g64x64n", 1, 9, 9, 64, 64, 3, 1, 1, G, True, "same", hint(64, 64, True), 0, (0, 64, 64, 0)),
    Row("g32x128w", 1, 8, 8, 64, 2, 1, 1, 0, ACT_NONE, False, "same", hint(32, 128), 0, (0, 32, 128, 1)),       # K = 2
    Row("g32x128n", 2, 7, 7, 64, 32, 3, 1, 1, S, False, "same", hint(32, 128, True), 0, (0, 32, 128, 0)),
    Row("g32x64w", 1, 9, 7, 128, 16, 1, 1, 0, E, False, "f32", hint(32, 64), 0, (0, 32, 64, 1)),
    Row("g32x64n", 1, 6, 10, 64, 32, 3, 1, 1, ACT_NONE, True, "same", hint(32, 64, True), 0, (0, 32, 64, 0)),
    # the scalar epilogue: output channel slice at offset 2 of a K + 2 wide buffer (not 16-byte aligned)
    Row("g64x64w_slice", 2, 10, 10, 64, 64, 3, 1, 1, S, True, "slice", hint(64, 64), 0, (0, 64, 64, 1)),
    Row("g128x64n_slice", 1, 6, 7, 128, 96, 1, 1, 0, ACT_NONE, False, "slice", hint(128, 64, True), 0, (0, 128, 64, 0)),
    # direct 3x3, first formulation (policy bit 4): TC 64 and TC 128
    Row("direct64", 1, 16, 32, 64, 64, 3, 1, 1, E, False, "same", 0, DIRECT_FIRST, (1, 64, 256, 1)),
    Row("direct128", 2, 32, 16, 128, 256, 3, 1, 1, S, True, "same", 0, DIRECT_FIRST, (1, 128, 256, 1)),
    # direct 3x3, row-reuse formulation (hint bit 25): TC 64 (K tail 48) and TC 128 (ragged channel tile K = 96)
    Row("rowreuse64", 1, 16, 16, 64, 48, 3, 1, 1, G, False, "same", ROW_REUSE, 0, (1, 64, 256, 0)),
    Row("rowreuse128", 1, 48, 16, 128, 96, 3, 1, 1, S, True, "same", ROW_REUSE, 0, (1, 128, 256, 0)),
    # the streaming head conv (pw_stream.hip): bias only, fp32 output, 16-bit inputs only
    Row("pw_stream", 2, 10, 10, 64, 32, 1, 1, 0, ACT_NONE, False, "f32", 0, 0, (2, 32, 128, 0), scale=False,
        dtypes=(torch.float16, torch.bfloat16)),
    # ConvTranspose2d(2, 2) output mode: K = 4 * 32 packed rows, default tile rules
    Row("convt2x2", 2, 6, 5, 64, 128, 1, 1, 0, ACT_NONE, False, "same", 0, 0, (0, 64, 64, 1), scale=False, convt=True),
]
ROWS = {r.name: r for r in VARIANTS}


def conv_args(L, row: Row, dtype: torch.dtype, ptrs=None):
    """The mtbt_conv_args of a row, as engine.Plan.conv fills them.  Without `ptrs` the pointers are fake (16-byte aligned, never
    dereferenced by mtbt_conv_kernel_choice), the output pointer offset like the real slice."""
    code = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    out_code = L.F32 if row.out == "f32" else code
    oes = 4 if out_code == L.F32 else 2
    a = L.ConvArgs()
    if ptrs is None:
        ptrs = dict(x=0x100000, w=0x200000, y=0x300000 + row.c0 * oes, scale=0x400000 if row.scale else None, shift=0x500000,
                    res=0x600000 if row.res else None)
    a.x, a.w, a.y = ptrs["x"], ptrs["w"], ptrs["y"]
    a.scale, a.shift, a.res = ptrs["scale"], ptrs["shift"], ptrs["res"]
    a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad = row.N, row.H, row.W, row.C, row.K, row.k, row.k, row.stride, row.pad
    a.Ho, a.Wo = row.Ho, row.Wo
    a.x_pixel_stride, a.x_batch_stride = row.C, row.H * row.W * row.C
    a.y_pixel_stride, a.y_batch_stride = row.pitch, row.Ho * row.Wo * row.pitch
    if row.convt:
        a.y_pixel_stride, a.y_batch_stride = row.K // 4, 4 * row.Ho * row.Wo * row.K // 4
    a.res_pixel_stride, a.res_batch_stride = (row.K, row.Ho * row.Wo * row.K) if row.res else (0, 0)
    a.dtype, a.out_dtype, a.act = code, out_code, row.act
    a.out_mode = L.OUT_CONVT2X2 if row.convt else L.OUT_NHWC
    a.tile_hint, a.policy = row.hint, row.policy
    return a


def kernel_choice(L, lib, a) -> Tuple[int, int, int, int]:
    import ctypes as C
    out = (C.c_int32 * 4)()
    rc = lib.mtbt_conv_kernel_choice(C.byref(a), out)
    assert rc == 0, rc
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------------------
# Exact operands: small integers, a power-of-two scale and a dyadic shift make every product and partial sum exact in fp32, so a
# kernel's result does not depend on its accumulation order and must equal the exact result rounded ONCE.
# ------------------------------------------------------------------------------------------------------------------------------------
def exact_operands(row, dtype, g, target=4000.0, scale_pow=None, shift_step=0.25):
    """Integer x in [-8, 8] ([-64, 64] for rows without a scale vector), w in [-8, 8] (exact in every storage type), a per-channel
    power-of-two scale putting the outputs near `target`, a shift in quarter steps and an integer residual rounded to the storage type.
    Returns the operands and the exact fp64 result."""
    xr = 8 if row.scale else 64
    x = torch.randint(-xr, xr + 1, (row.N, row.C, row.H, row.W), generator=g).double()
    w = torch.randint(-8, 9, (row.K, row.C, row.k, row.k), generator=g).double()
    if scale_pow is None:
        scale_pow = round(math.log2(target / (24.0 * math.sqrt(row.C * row.k * row.k))))
    scale = (2.0 ** (scale_pow + torch.randint(0, 2, (row.K,), generator=g))).float() if row.scale else None
    shift = torch.randint(-64, 65, (row.K,), generator=g).float() * shift_step
    res = storage(torch.randint(-1000, 1001, (row.N, row.K, row.Ho, row.Wo), generator=g).double(), dtype) if row.res else None
    acc = F.conv2d(x, w, None, row.stride, row.pad)
    exact = acc * (scale.double().view(1, -1, 1, 1) if scale is not None else 1.0) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        exact = exact + res
    assert torch.equal(exact.float().double(), exact), "the exact result must be an fp32 value"
    return x, w, scale, shift, res, exact


def rounded_once(exact, out_dt):
    """The exact fp32 result rounded once into the output type (from fp32, as the kernel does); fp16 saturates at +-65504 (common.h)."""
    e = exact.float()
    if out_dt == torch.float16:
        e = e.clamp(-65504.0, 65504.0)
    return e.to(out_dt).double()


# ------------------------------------------------------------------------------------------------------------------------------------
# Training variant table: the same kernels with the training epilogue bodies of conv_epilogue.h.
#   mode "y2":    the pre-activation as a second output next to y = act(.) (+ res)              (MODE 1 of the fast body)
#   mode "deriv": y = affine * act'(res), act one of the D* codes; the residual is the pre-activation z  (MODE 2)
#   mode "accum": the residual IS the output buffer (a gradient accumulating in place)           (MODE 0 with res == y)
# colsum: per-channel sums of the stored output from the same launch (the SUMS bodies: ACT_NONE and ACT_DGELU_POLY; everything else the
# general body; not on the 96-channel tiles).
# Layouts: where y / y2 / res live, as (extra channels of the buffer, first channel of the view, extra pixel rows per image).  y2 has no
# strides of its own in mtbt_conv_args: it shares y's pitch and batch stride.
#   dense     plain NHWC tensors;
#   slice16   16-byte-aligned channel slices of wider buffers, res with ANOTHER pitch than y: still the fast bodies;
#   batchgap  a gap after every image (y_batch_stride > Ho * Wo * pitch; res with another gap): y_linear is false, the general body;
#   slice2    y at channel offset 2 of a K + 2 wide buffer (misaligned: the scalar body), y2 aligned in its own buffer of that pitch;
#   f32       fp32 y and y2 from 16-bit operands (the general body).
# ------------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {
    "dense": dict(y=(0, 0, 0), y2=(0, 0, 0), res=(0, 0, 0)),
    "slice16": dict(y=(24, 8, 0), y2=(24, 16, 0), res=(40, 24, 0)),
    "batchgap": dict(y=(0, 0, 3), y2=(0, 0, 3), res=(0, 0, 5)),
    "slice2": dict(y=(2, 2, 0), y2=(2, 0, 0), res=(0, 0, 0)),
    "f32": dict(y=(0, 0, 0), y2=(0, 0, 0), res=(0, 0, 0)),
}


@dataclass(frozen=True)
class TrainRow(Row):
    mode: str = "y2"         # "y2" | "deriv" | "accum"
    colsum: bool = False
    layout: str = "dense"

    def view(self, which):
        """(buffer width in channels, first channel, pixel rows per image) of "y" / "y2" / "res"."""
        wpad, c0, gap = LAYOUTS[self.layout]["y" if which == "res" and self.mode == "accum" else which]
        return self.K + wpad, c0, self.Ho * self.Wo + gap


def _t(name, N, H, W, C, K, k, stride, pad, act, res, hint_, expect, mode, layout="dense", colsum=False, policy=0):
    return TrainRow(name, N, H, W, C, K, k, stride, pad, act, res, "f32" if layout == "f32" else "same", hint_, policy, expect,
                    mode=mode, colsum=colsum, layout=layout)


DS, DE, DG, DP = ACT_DSILU, ACT_DELU, ACT_DGELU, ACT_DGELU_POLY
CS_TILES = [(128, 128), (128, 64), (64, 128), (64, 64), (32, 128), (32, 64)]       # the tiles that allow column sums
TRAIN_VARIANTS = [
    # ---- y2: every tile; 2 x 9 x 7 = 126 pixels is ragged for both pixel tiles and leaves 14 rows in the last slab; K = TC + 8 a second,
    # nearly empty channel tile.  NONE / GELU / GELU_POLY: the fast body; SILU / ELU: the general one.
    _t("y2_128x128w", 2, 9, 7, 64, 128, 1, 1, 0, GP, False, hint(128, 128), (0, 128, 128, 1), "y2"),
    _t("y2_128x64n", 2, 9, 7, 128, 136, 1, 1, 0, G, True, hint(128, 64, True), (0, 128, 64, 0), "y2"),
    _t("y2_96x128n", 1, 10, 10, 64, 96, 3, 1, 1, ACT_NONE, True, hint(96, 128, True), (0, 96, 128, 0), "y2"),
    _t("y2_96x64w", 2, 9, 7, 64, 104, 1, 1, 0, GP, False, hint(96, 64), (0, 96, 64, 1), "y2"),
    _t("y2_64x128w", 2, 9, 7, 128, 64, 1, 1, 0, S, False, hint(64, 128), (0, 64, 128, 1), "y2"),
    _t("y2_64x64n_3x3", 1, 16, 16, 64, 64, 3, 1, 1, GP, False, hint(64, 64, True), (0, 64, 64, 0), "y2"),   # 16-aligned map: not direct
    _t("y2_32x128n", 1, 3, 5, 64, 32, 1, 1, 0, G, False, hint(32, 128, True), (0, 32, 128, 0), "y2"),      # 15 pixels in all
    _t("y2_32x64w", 2, 9, 7, 64, 40, 1, 1, 0, E, True, hint(32, 64), (0, 32, 64, 1), "y2"),
    _t("y2_slice16", 2, 9, 7, 64, 128, 1, 1, 0, GP, True, hint(128, 64), (0, 128, 64, 1), "y2", "slice16"),
    _t("y2_batchgap", 2, 9, 7, 64, 64, 1, 1, 0, G, True, hint(64, 64), (0, 64, 64, 1), "y2", "batchgap"),
    _t("y2_slice2", 2, 6, 5, 64, 64, 1, 1, 0, GP, True, hint(64, 128), (0, 64, 128, 1), "y2", "slice2"),
    _t("y2_f32", 2, 9, 7, 64, 96, 1, 1, 0, G, False, hint(96, 64, True), (0, 96, 64, 0), "y2", "f32"),
    # ---- deriv: every tile; DSILU / DELU / DGELU_POLY: the fast body; DGELU: the general one; each on a PERM tile and on 96x64
    _t("d_128x128n", 2, 9, 7, 64, 128, 1, 1, 0, DP, True, hint(128, 128, True), (0, 128, 128, 0), "deriv"),
    _t("d_128x64w", 2, 9, 7, 128, 136, 1, 1, 0, DS, True, hint(128, 64), (0, 128, 64, 1), "deriv"),
    _t("d_96x128w", 2, 9, 7, 128, 96, 1, 1, 0, DE, True, hint(96, 128), (0, 96, 128, 1), "deriv"),
    _t("d_96x64n_dp", 2, 9, 7, 64, 96, 1, 1, 0, DP, True, hint(96, 64, True), (0, 96, 64, 0), "deriv"),
    _t("d_96x64w_ds", 1, 7, 9, 64, 104, 1, 1, 0, DS, True, hint(96, 64), (0, 96, 64, 1), "deriv"),
    _t("d_96x64w_de", 2, 9, 7, 64, 96, 1, 1, 0, DE, True, hint(96, 64), (0, 96, 64, 1), "deriv"),
    _t("d_96x64n_dg", 1, 3, 5, 64, 96, 1, 1, 0, DG, True, hint(96, 64, True), (0, 96, 64, 0), "deriv"),     # 15 pixels in all
    _t("d_64x128n", 2, 9, 7, 128, 72, 1, 1, 0, DG, True, hint(64, 128, True), (0, 64, 128, 0), "deriv"),
    _t("d_64x64w_3x3", 1, 16, 16, 64, 64, 3, 1, 1, DP, True, hint(64, 64), (0, 64, 64, 1), "deriv"),        # 16-aligned map: not direct
    _t("d_32x128w", 2, 9, 7, 64, 32, 1, 1, 0, DE, True, hint(32, 128), (0, 32, 128, 1), "deriv"),
    _t("d_32x64n", 2, 9, 7, 64, 40, 1, 1, 0, DS, True, hint(32, 64, True), (0, 32, 64, 0), "deriv"),
    _t("d_slice16", 2, 9, 7, 64, 128, 1, 1, 0, DP, True, hint(128, 128), (0, 128, 128, 1), "deriv", "slice16"),
    _t("d_batchgap", 2, 9, 7, 64, 64, 1, 1, 0, DS, True, hint(64, 64), (0, 64, 64, 1), "deriv", "batchgap"),
    _t("d_slice2", 2, 6, 5, 64, 64, 1, 1, 0, DE, True, hint(64, 128), (0, 64, 128, 1), "deriv", "slice2"),
    _t("d_f32", 2, 9, 7, 64, 128, 1, 1, 0, DP, True, hint(128, 64), (0, 128, 64, 1), "deriv", "f32"),
    # column sums from the DGELU_POLY launch (d fc1.bias): the SUMS body on every tile that allows them; DGELU once (the general body)
    *[_t(f"d_cs_{tc}x{tp}", 2, 9, 7, 64, tc, 1, 1, 0, DP, True, hint(tc, tp, narrow=(i % 2 == 1)), (0, tc, tp, 1 - i % 2), "deriv",
         colsum=True) for i, (tc, tp) in enumerate(CS_TILES)],
    _t("d_cs_dgelu", 2, 9, 7, 64, 128, 1, 1, 0, DG, True, hint(128, 64), (0, 128, 64, 1), "deriv", colsum=True),
    # ---- accum: res is y.  A wide and a narrow implicit-GEMM tile per TC 128 / 64 / 32, 96x64, the 2x2 / stride-2 dgrad form, both direct
    # formulations at TC 64 / 128 (4 and 8 slabs per wave).  The smallest shapes that have that: the fp32 rows rest on ACC * mag alone, the order
    # of a random walk and no worst case -- over the 131072 outputs of a 2 x 32 x 16 map with a 1152-term reduction one output reached 1.03 of its
    # bound on the direct kernel, and a plain sequential fp32 sum of the same operands 1.02 (forwards) and 1.07 (backwards).
    _t("a_128x128w", 2, 9, 7, 64, 128, 1, 1, 0, ACT_NONE, True, hint(128, 128), (0, 128, 128, 1), "accum"),
    _t("a_128x64n", 2, 9, 7, 128, 136, 1, 1, 0, ACT_NONE, True, hint(128, 64, True), (0, 128, 64, 0), "accum"),
    _t("a_64x128n", 2, 9, 7, 64, 64, 1, 1, 0, ACT_NONE, True, hint(64, 128, True), (0, 64, 128, 0), "accum"),
    _t("a_64x64w_3x3", 1, 10, 10, 64, 72, 3, 1, 1, ACT_NONE, True, hint(64, 64), (0, 64, 64, 1), "accum"),
    _t("a_32x128w", 2, 9, 7, 128, 32, 1, 1, 0, ACT_NONE, True, hint(32, 128), (0, 32, 128, 1), "accum"),
    _t("a_32x64n", 1, 3, 5, 64, 40, 1, 1, 0, ACT_NONE, True, hint(32, 64, True), (0, 32, 64, 0), "accum"),
    _t("a_96x64w", 2, 9, 7, 64, 96, 1, 1, 0, ACT_NONE, True, hint(96, 64), (0, 96, 64, 1), "accum"),
    _t("a_down2x2", 2, 10, 6, 64, 128, 2, 2, 0, ACT_NONE, True, hint(128, 64), (0, 128, 64, 1), "accum"),
    _t("a_direct64", 1, 16, 32, 64, 64, 3, 1, 1, ACT_NONE, True, 0, (1, 64, 256, 1), "accum", policy=DIRECT_FIRST),
    _t("a_direct128", 2, 16, 16, 64, 128, 3, 1, 1, ACT_NONE, True, 0, (1, 128, 256, 1), "accum", policy=DIRECT_FIRST),
    _t("a_rowreuse64", 1, 16, 16, 64, 48, 3, 1, 1, ACT_NONE, True, ROW_REUSE, (1, 64, 256, 0), "accum"),
    _t("a_rowreuse128", 1, 48, 16, 128, 96, 3, 1, 1, ACT_NONE, True, ROW_REUSE, (1, 128, 256, 0), "accum"),
    # column sums of the raw conv (the ACT_NONE SUMS body), accumulating in place
    *[_t(f"a_cs_{tc}x{tp}", 2, 9, 7, 64, tc, 1, 1, 0, ACT_NONE, True, hint(tc, tp, narrow=(i % 2 == 0)), (0, tc, tp, i % 2), "accum",
         colsum=True) for i, (tc, tp) in enumerate(CS_TILES)],
    # the same on the direct kernels: the only road to the fast slab body there (with column sums; without, MODE 0 stores straight from the
    # accumulators), whose residual prefetch runs one slab ahead of the aliasing stores
    _t("a_cs_direct64", 1, 16, 32, 64, 64, 3, 1, 1, ACT_NONE, True, 0, (1, 64, 256, 1), "accum", colsum=True, policy=DIRECT_FIRST),
    _t("a_cs_direct128", 2, 16, 16, 64, 128, 3, 1, 1, ACT_NONE, True, 0, (1, 128, 256, 1), "accum", colsum=True, policy=DIRECT_FIRST),
    _t("a_cs_rowreuse64", 1, 16, 16, 64, 48, 3, 1, 1, ACT_NONE, True, ROW_REUSE, (1, 64, 256, 0), "accum", colsum=True),
    _t("a_cs_rowreuse128", 2, 16, 16, 64, 96, 3, 1, 1, ACT_NONE, True, ROW_REUSE, (1, 128, 256, 0), "accum", colsum=True),
]
TRAIN_ROWS = {r.name: r for r in TRAIN_VARIANTS}


def train_conv_args(L, row: TrainRow, dtype: torch.dtype):
    """The mtbt_conv_args of a training row with fake pointers (never dereferenced by mtbt_conv_kernel_choice), offset, pitched and
    strided like the real views; the GPU tests fill theirs through engine.Plan.conv from the same TrainRow.view."""
    code = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    out_code = L.F32 if row.layout == "f32" else code
    oes, es = (4 if out_code == L.F32 else 2), (4 if code == L.F32 else 2)
    a = conv_args(L, row, dtype, ptrs=dict(x=0x100000, w=0x200000, y=0, scale=0x400000 if row.scale else None, shift=0x500000, res=None))
    yw, yc, yr = row.view("y")
    a.y, a.y_pixel_stride, a.y_batch_stride = 0x300000 + yc * oes, yw, yr * yw
    if row.mode == "y2":
        assert row.view("y2")[0] == yw and row.view("y2")[2] == yr, "y2 shares y's pitch and batch stride"
        a.y2 = 0x700000 + row.view("y2")[1] * oes
    if row.res:
        rw, rc, rr = row.view("res")
        a.res = a.y if row.mode == "accum" else 0x600000 + rc * es
        a.res_pixel_stride, a.res_batch_stride = rw, rr * rw
    if row.colsum:
        a.colsum, a.colsum_ws, a.colsum_ws_bytes = 0x800000, 0x900000, 1 << 30
    return a


def train_row_reference(row, dtype, seed=0):
    """A training row as the parity tests build it: storage-precision operands, fp32 scale / shift.  Returns the
    operands and {"y": (ref, bound), "y2": (ref, bound)} (y2 only in mode "y2").  Mode "accum": res is what y holds before the launch."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, row.name)))
    x = storage(torch.randn(row.N, row.C, row.H, row.W, generator=g), dtype)
    w = storage(torch.randn(row.K, row.C, row.k, row.k, generator=g) / (row.C * row.k * row.k) ** 0.5, dtype)
    scale = torch.rand(row.K, generator=g) + 0.5
    shift = torch.randn(row.K, generator=g) * 0.1
    res = storage(torch.randn(row.N, row.K, row.Ho, row.Wo, generator=g), dtype) if row.res else None
    out_dt = torch.float32 if row.layout == "f32" else dtype
    acc, mag = conv_sums(x, w, row.stride, row.pad)
    refs = {}
    if row.mode == "deriv":
        refs["y"] = deriv_ref(acc, mag, scale, shift, row.act, res, out_dt)
    else:
        refs["y"] = affine_act_ref(acc, mag, scale, shift, row.act, res, out_dt)
    if row.mode == "y2":
        refs["y2"] = preact_ref(acc, mag, scale, shift, out_dt)
    return (x, w, scale, shift, res), refs


# ------------------------------------------------------------------------------------------------------------------------------------
# Depthwise variant table (csrc/dwconv.inc: mtbt_dwconv_nhwc, mtbt_dwconv_nhwc_train, mtbt_dwconv3x3_mult_nhwc);
# tests/test_gpu_dwconv_variants.py runs it.  Each row: shape (C = the channels of x), kernel size, form (LayerNorm or scale / shift + act),
# the training extras (raw = the LayerNorm input as a second output; res = "buf" a residual tensor / "y" the residual IS the output), the
# depth multiplier M (0 = the plain entry) and, per storage width, the mtbt_dwconv_kernel_choice tuple it must reach:
#   (tile height, tile width, outputs per lane row, MAXCH, FULL, compiled activation (-1 = runtime), tiles, gridDim.x, gridDim.y).
# e16 holds for f16 and bf16 (16-wide tiles, activation constants, FULL instantiations), e32 for f32 (8-wide tiles, bounds-checked,
# runtime activation); None = the row does not run in that width (the walk rows are sized per width).
# walk: the persistent workgroups take further tiles (one chunk: some workgroup runs a first, a middle and a last tile).
# No tolerance of its own: the scale / shift form uses affine_act_ref, the LayerNorm form ln_bound with v_err = ACC sum |x w| + EPI |bias|
# (as test_fp16_dwconv7_layernorm), raw the bound of conv + bias rounded once (preact_ref with the bias as shift).
# ------------------------------------------------------------------------------------------------------------------------------------
DW_EPS = 1e-6
DW_FIELDS = ("th", "tw", "xb", "maxch", "full", "act", "tiles", "gx", "gy")


@dataclass(frozen=True)
class DwRow:
    name: str
    N: int
    C: int
    H: int
    W: int
    k: int
    ln: bool
    act: int
    e16: Optional[Tuple[int, ...]]
    e32: Optional[Tuple[int, ...]]
    raw: bool = False
    res: str = ""            # "" | "buf" | "y"
    M: int = 0
    walk: bool = False

    @property
    def Co(self):
        return self.C * max(self.M, 1)

    @property
    def dtypes(self):
        return tuple(d for d in DTYPES if self.expect(d) is not None)

    def expect(self, dtype):
        return self.e32 if dtype == torch.float32 else self.e16

    def field(self, dtype, name):
        return self.expect(dtype)[DW_FIELDS.index(name)]


def _ln(name, shape, k, e16, e32, raw=False, walk=False):
    return DwRow(name, *shape, k, True, ACT_NONE, e16, e32, raw=raw, walk=walk)


def _af(name, shape, k, act, e16, e32, res="", walk=False):
    return DwRow(name, *shape, k, False, act, e16, e32, res=res, walk=walk)


def _mu(name, shape, M, act, e16, e32):
    return DwRow(name, *shape, 3, False, act, e16, e32, M=M)


N_, SI = ACT_NONE, ACT_SILU
DW_VARIANTS = [
    # ---- LayerNorm form, 7x7: MAXCH 1 / 2 / 3 / 6, each ragged (_r) and in whole tiles (_f: the FULL instantiation of the 16-bit types); a last
    # chunk of 8 channels at C = 8, 136, 264, 392, 520, 648; the six-chunk kernel with 4 (392), 5 (520) and 6 (648, 768) live chunks
    _ln("ln7_c96_r", (2, 96, 9, 11), 7, (4, 16, 8, 1, 0, 0, 6, 8, 1), (4, 8, 8, 1, 0, 0, 12, 16, 1), raw=True),
    _ln("ln7_c8_f", (2, 8, 8, 16), 7, (4, 16, 8, 1, 1, 0, 4, 8, 1), (4, 8, 8, 1, 0, 0, 8, 8, 1)),
    _ln("ln7_c136_r", (2, 136, 7, 18), 7, (4, 16, 8, 2, 0, 0, 8, 8, 1), (4, 8, 8, 2, 0, 0, 12, 16, 1), raw=True),
    _ln("ln7_c256_f", (2, 256, 8, 32), 7, (4, 16, 8, 2, 1, 0, 8, 8, 1), (4, 8, 8, 2, 0, 0, 16, 16, 1)),
    _ln("ln7_c264_r", (2, 264, 5, 9), 7, (4, 8, 4, 3, 0, 0, 8, 8, 1), (4, 4, 4, 3, 0, 0, 12, 16, 1)),
    _ln("ln7_c384_f", (2, 384, 8, 8), 7, (4, 8, 4, 3, 1, 0, 4, 8, 1), (4, 4, 4, 3, 0, 0, 8, 8, 1), raw=True),
    _ln("ln7_c392_r", (2, 392, 6, 7), 7, (4, 8, 4, 6, 0, 0, 4, 8, 1), (4, 4, 4, 6, 0, 0, 8, 8, 1), raw=True),
    _ln("ln7_c520_f", (2, 520, 4, 16), 7, (4, 8, 4, 6, 1, 0, 4, 8, 1), (4, 4, 4, 6, 0, 0, 8, 8, 1)),
    _ln("ln7_c648_r", (1, 648, 3, 15), 7, (4, 8, 4, 6, 0, 0, 2, 8, 1), (4, 4, 4, 6, 0, 0, 4, 8, 1)),
    _ln("ln7_c768_f", (2, 768, 4, 8), 7, (4, 8, 4, 6, 1, 0, 2, 8, 1), (4, 4, 4, 6, 0, 0, 4, 8, 1), raw=True),
    _ln("ln7_c96_1x1", (2, 96, 1, 1), 7, (4, 16, 8, 1, 0, 0, 2, 8, 1), (4, 8, 8, 1, 0, 0, 2, 8, 1), raw=True),
    # ---- LayerNorm form, 3x3: the same cells; H = W = 2, H = 3 = tile - 1, W = 15 / 7 / 3 = tile - 1 of the 16 / 8 / 4 wide tiles
    _ln("ln3_c8_r", (2, 8, 5, 17), 3, (4, 16, 8, 1, 0, 0, 8, 8, 1), (4, 8, 8, 1, 0, 0, 12, 16, 1), raw=True),
    _ln("ln3_c96_f", (2, 96, 4, 32), 3, (4, 16, 8, 1, 1, 0, 4, 8, 1), (4, 8, 8, 1, 0, 0, 8, 8, 1)),
    _ln("ln3_c136_f", (2, 136, 8, 16), 3, (4, 16, 8, 2, 1, 0, 4, 8, 1), (4, 8, 8, 2, 0, 0, 8, 8, 1)),
    _ln("ln3_c192_r", (2, 192, 3, 15), 3, (4, 16, 8, 2, 0, 0, 2, 8, 1), (4, 8, 8, 2, 0, 0, 4, 8, 1), raw=True),
    _ln("ln3_c264_f", (2, 264, 4, 24), 3, (4, 8, 4, 3, 1, 0, 6, 8, 1), (4, 4, 4, 3, 0, 0, 12, 16, 1), raw=True),
    _ln("ln3_c320_r", (2, 320, 3, 3), 3, (4, 8, 4, 3, 0, 0, 2, 8, 1), (4, 4, 4, 3, 0, 0, 2, 8, 1)),
    _ln("ln3_c448_f", (2, 448, 8, 8), 3, (4, 8, 4, 6, 1, 0, 4, 8, 1), (4, 4, 4, 6, 0, 0, 8, 8, 1)),
    _ln("ln3_c640_r", (2, 640, 2, 2), 3, (4, 8, 4, 6, 0, 0, 2, 8, 1), (4, 4, 4, 6, 0, 0, 2, 8, 1), raw=True),
    _ln("ln3_c648_f", (1, 648, 4, 16), 3, (4, 8, 4, 6, 1, 0, 2, 8, 1), (4, 4, 4, 6, 0, 0, 4, 8, 1), raw=True),
    _ln("ln3_c768_r", (2, 768, 5, 6), 3, (4, 8, 4, 6, 0, 0, 4, 8, 1), (4, 4, 4, 6, 0, 0, 8, 8, 1)),
    # ---- LayerNorm form, walk rows of the 16-bit types: 1040 tiles on 512 workgroups (one chunk: first, middle and last tile), 529 on 512
    # (two, three chunks), 289 on 256 (six-chunk kernel, five live); 3x3 with one chunk (every type) and three
    _ln("w16_ln7_c96", (1, 96, 103, 635), 7, (4, 16, 8, 1, 0, 0, 1040, 512, 1), None, raw=True, walk=True),
    _ln("w16_ln7_c192", (1, 192, 92, 361), 7, (4, 16, 8, 2, 0, 0, 529, 512, 1), None, walk=True),
    _ln("w16_ln7_c384", (1, 384, 90, 181), 7, (4, 8, 4, 3, 0, 0, 529, 512, 1), None, raw=True, walk=True),
    _ln("w16_ln7_c520", (1, 520, 66, 131), 7, (4, 8, 4, 6, 0, 0, 289, 256, 1), None, walk=True),
    _ln("w_ln3_c96", (1, 96, 103, 635), 3, (4, 16, 8, 1, 0, 0, 1040, 512, 1), (4, 8, 8, 1, 0, 0, 2080, 1024, 1), walk=True),
    _ln("w16_ln3_c384", (1, 384, 90, 181), 3, (4, 8, 4, 3, 0, 0, 529, 512, 1), None, raw=True, walk=True),
    # ---- LayerNorm form, walk rows of fp32 (4 x 8 and 4 x 4 tiles)
    _ln("w32_ln7_c96", (1, 96, 103, 315), 7, None, (4, 8, 8, 1, 0, 0, 1040, 512, 1), walk=True),
    _ln("w32_ln7_c192", (1, 192, 66, 131), 7, None, (4, 8, 8, 2, 0, 0, 289, 256, 1), raw=True, walk=True),
    _ln("w32_ln7_c384", (1, 384, 90, 90), 7, None, (4, 4, 4, 3, 0, 0, 529, 512, 1), walk=True),
    _ln("w32_ln7_c768", (1, 768, 90, 90), 7, None, (4, 4, 4, 6, 0, 0, 529, 512, 1), raw=True, walk=True),
    # ---- scale / shift form, 7x7: C <= 128 and the chunks as 2 / 3 grid rows with a ragged last chunk; full-width tiles (W a multiple of the
    # tile width) and half-width ones; the activation as the NONE / SILU constant and at run time (ELU); no residual, a residual tensor, res is y
    _af("af7_c96_f", (2, 96, 8, 32), 7, N_, (4, 16, 8, 1, 1, 0, 8, 8, 1), (4, 8, 8, 1, 0, -1, 16, 16, 1)),
    _af("af7_c128_r", (2, 128, 9, 21), 7, SI, (4, 8, 4, 1, 0, 1, 18, 24, 1), (4, 4, 4, 1, 0, -1, 36, 40, 1), res="buf"),
    _af("af7_c192_hf", (2, 192, 8, 24), 7, E, (4, 8, 4, 1, 1, -1, 12, 8, 2), (4, 8, 8, 1, 0, -1, 12, 8, 2)),
    _af("af7_c264_r", (2, 264, 7, 19), 7, N_, (4, 8, 4, 1, 0, 0, 12, 8, 3), (4, 4, 4, 1, 0, -1, 20, 8, 3), res="y"),
    _af("af7_c328_f", (1, 328, 12, 16), 7, SI, (4, 16, 8, 1, 1, 1, 3, 8, 3), (4, 8, 8, 1, 0, -1, 6, 8, 3)),
    _af("af7_c8_r", (2, 8, 3, 15), 7, N_, (4, 8, 4, 1, 0, 0, 4, 8, 1), (4, 4, 4, 1, 0, -1, 8, 8, 1), res="buf"),
    _af("af7_c64_r16", (2, 64, 6, 32), 7, E, (4, 16, 8, 1, 0, -1, 8, 8, 1), (4, 8, 8, 1, 0, -1, 16, 16, 1), res="y"),
    # ---- scale / shift form, 3x3 (always the full-width tile); a 1 x 2 image
    _af("af3_c64_r", (2, 64, 3, 7), 3, E, (4, 16, 8, 1, 0, -1, 2, 8, 1), (4, 8, 8, 1, 0, -1, 2, 8, 1)),
    _af("af3_c128_f", (2, 128, 8, 16), 3, N_, (4, 16, 8, 1, 1, 0, 4, 8, 1), (4, 8, 8, 1, 0, -1, 8, 8, 1), res="y"),
    _af("af3_c192_r", (2, 192, 6, 17), 3, SI, (4, 16, 8, 1, 0, 1, 8, 8, 2), (4, 8, 8, 1, 0, -1, 12, 8, 2), res="buf"),
    _af("af3_c264_f", (2, 264, 4, 32), 3, N_, (4, 16, 8, 1, 1, 0, 4, 8, 3), (4, 8, 8, 1, 0, -1, 8, 8, 3), res="buf"),
    _af("af3_c256_1x2", (3, 256, 1, 2), 3, SI, (4, 16, 8, 1, 0, 1, 3, 8, 2), (4, 8, 8, 1, 0, -1, 3, 8, 2)),
    _af("af3_c392_f", (1, 392, 8, 16), 3, E, (4, 16, 8, 1, 1, -1, 2, 8, 4), (4, 8, 8, 1, 0, -1, 4, 8, 4), res="y"),
    # ---- scale / shift form at C <= 128, walk rows: act none, so that the bit-exact check runs the very kernel of the parity check
    _af("w16_af7_full", (1, 72, 103, 640), 7, N_, (4, 16, 8, 1, 0, 0, 1040, 512, 1), None, walk=True),
    _af("w16_af7_half", (1, 72, 103, 315), 7, N_, (4, 8, 4, 1, 0, 0, 1040, 512, 1), None, res="y", walk=True),
    _af("w16_af3", (1, 72, 103, 635), 3, N_, (4, 16, 8, 1, 0, 0, 1040, 512, 1), None, res="buf", walk=True),
    _af("w32_af7_full", (1, 72, 103, 320), 7, N_, None, (4, 8, 8, 1, 0, -1, 1040, 512, 1), walk=True),
    _af("w32_af7_half", (1, 72, 103, 237), 7, N_, None, (4, 4, 4, 1, 0, -1, 1560, 768, 1), res="y", walk=True),
    _af("w32_af3", (1, 72, 103, 635), 3, N_, None, (4, 8, 8, 1, 0, -1, 2080, 1024, 1), res="buf", walk=True),
    # ---- depth multiplier: M = 1 / 2, C = 128 / 256, ragged and whole tiles, every activation choice
    _mu("mu1_c128_r", (2, 128, 5, 9), 1, SI, (4, 16, 8, 1, 0, 1, 4, 8, 1), (4, 8, 8, 1, 0, -1, 8, 8, 1)),
    _mu("mu2_c128_f", (2, 128, 8, 16), 2, N_, (4, 16, 8, 1, 1, 0, 4, 8, 2), (4, 8, 8, 1, 0, -1, 8, 8, 2)),
    _mu("mu1_c256_f", (1, 256, 4, 32), 1, E, (4, 16, 8, 1, 1, -1, 2, 8, 2), (4, 8, 8, 1, 0, -1, 4, 8, 2)),
    _mu("mu2_c256_r", (2, 256, 7, 10), 2, SI, (4, 16, 8, 1, 0, 1, 4, 8, 4), (4, 8, 8, 1, 0, -1, 8, 8, 4)),
    _mu("mu2_c128_n", (2, 128, 6, 11), 2, N_, (4, 16, 8, 1, 0, 0, 4, 8, 2), (4, 8, 8, 1, 0, -1, 8, 8, 2)),
]
DW_ROWS = {r.name: r for r in DW_VARIANTS}


def dw_choice(L, lib, row: DwRow, dtype) -> Tuple[int, ...]:
    """What the entry point of this row would launch (host-only query)."""
    import ctypes as C
    code = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
    out = (C.c_int32 * 9)()
    if row.M:
        rc = lib.mtbt_dwconv3x3_mult_kernel_choice(row.N, row.H, row.W, row.C, row.M, row.act, code, out)
    else:
        rc = lib.mtbt_dwconv_kernel_choice(row.N, row.H, row.W, row.C, row.k, int(row.ln), row.act, code, out)
    assert rc == 0, rc
    return tuple(out)


def storage16(t: torch.Tensor) -> torch.Tensor:
    """t rounded so that it is exact in bf16 AND in fp16 (bf16's 8 significant bits; below fp16's normal range the fp16 subnormal grid, which
    leaves at most 7): the big walk rows share one reference between the two 16-bit types."""
    s = t.to(torch.bfloat16).to(torch.float16)
    assert torch.equal(s.double(), s.to(torch.bfloat16).double())
    return s.double()


def dw_sums(x: torch.Tensor, w: torch.Tensor):
    """(sum x*w, sum |x*w|) of a depthwise k x k conv (stride 1, pad k/2) in fp64, by shift-and-add over the taps.  x [N,C,H,W], w [Co,k,k]
    with Co = M * C: output channel j reads input channel j mod C (M = 1: the plain depthwise conv)."""
    (N, C, H, W), k = x.shape, w.shape[-1]
    if w.shape[0] != C:
        x = x.repeat(1, w.shape[0] // C, 1, 1)
    xp = F.pad(x, (k // 2,) * 4)
    xa, wa = xp.abs(), w.abs()
    acc, mag = torch.zeros_like(x), torch.zeros_like(x)
    for ky in range(k):
        for kx in range(k):
            acc.addcmul_(xp[:, :, ky:ky + H, kx:kx + W], w[:, ky, kx].view(1, -1, 1, 1))
            mag.addcmul_(xa[:, :, ky:ky + H, kx:kx + W], wa[:, ky, kx].view(1, -1, 1, 1))
    return acc, mag


def dw_ln_ref(acc, mag, bias, lw, lb, out_dtype, stat_channels=None):
    """LayerNorm form from the conv sums (NCHW): {"y": LayerNorm over C of v = conv + bias, "raw": v rounded once}, each (ref, bound), NCHW.
    stat_channels: a DEFECT for the sensitivity tests -- the statistics taken over that many leading channels only."""
    N, C, H, W = acc.shape
    b = bias.double().view(1, -1, 1, 1)
    v = (acc + b).permute(0, 2, 3, 1).reshape(-1, C)
    verr = (ACC * mag + EPI * b.abs()).permute(0, 2, 3, 1).reshape(-1, C).amax(-1, keepdim=True)
    if stat_channels is None:
        y = F.layer_norm(v, (C,), lw.double(), lb.double(), DW_EPS)
    else:
        m = v[:, :stat_channels].mean(-1, keepdim=True)
        var = ((v[:, :stat_channels] - m) ** 2).mean(-1, keepdim=True)
        y = (v - m) / torch.sqrt(var + DW_EPS) * lw.double() + lb.double()
    bnd = ln_bound(y, v, lw, lb, DW_EPS, verr, out_dtype)
    back = lambda t: t.reshape(N, H, W, C).permute(0, 3, 1, 2)
    return {"y": (back(y), back(bnd)), "raw": preact_ref(acc, mag, None, bias, out_dtype)}


def dw_operands(row: DwRow, dtype, seed=0):
    """Random operands of a row as the kernel reads them: x / w / res in storage precision (the 16-bit walk rows: exact in both 16-bit types),
    the per-channel vectors fp32.  Returns a dict; v0 / v1 / v2 are bias, ln weight, ln bias (LayerNorm form) or scale, shift, None."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, row.name)))
    st = (lambda t: storage(t, dtype)) if not (row.walk and dtype != torch.float32) else storage16
    Co, k = row.Co, row.k
    o = dict(x=st(torch.randn(row.N, row.C, row.H, row.W, generator=g)), w=st(torch.randn(Co, k, k, generator=g) / k))
    if row.ln:
        o.update(v0=torch.randn(Co, generator=g) * 0.1, v1=torch.rand(Co, generator=g) + 0.5, v2=torch.randn(Co, generator=g) * 0.1)
    else:
        o.update(v0=torch.rand(Co, generator=g) + 0.5, v1=torch.randn(Co, generator=g) * 0.1, v2=None)
    o["res"] = st(torch.randn(row.N, Co, row.H, row.W, generator=g)) if row.res else None
    return o


_dw_cache = {}


def dw_row_sums(row: DwRow, dtype, seed=0):
    """(operands, conv sums) of a row; the last row's are kept (the fp64 conv is the cost of a walk row: once per row and storage)."""
    key = (row.name, "16" if row.walk and dtype != torch.float32 else DNAME[dtype], seed)
    if key not in _dw_cache:
        _dw_cache.clear()
        o = dw_operands(row, dtype, seed)
        _dw_cache[key] = (o, dw_sums(o["x"], o["w"]))
    return _dw_cache[key]


def dw_row_reference(row: DwRow, dtype, seed=0):
    """Operands and {"y": (ref, bound)[, "raw": (ref, bound)]} of a row, NCHW fp64: what the GPU parity test checks with `check`."""
    o, (acc, mag) = dw_row_sums(row, dtype, seed)
    if row.ln:
        refs = dw_ln_ref(acc, mag, o["v0"], o["v1"], o["v2"], dtype)
        if not row.raw:
            del refs["raw"]
        return o, refs
    return o, {"y": affine_act_ref(acc, mag, o["v0"], o["v1"], row.act, o["res"], dtype)}


def dw_exact_operands(row: DwRow, dtype, seed=0, target=4000.0):
    """Integer operands of a row: x, w in [-8, 8] (exact in every storage type); every product and partial sum is exact in fp32.
    LayerNorm form: a bias in quarter steps up to +-2000 (so that conv + bias needs rounding in the 16-bit types), LayerNorm vectors as in
    dw_operands; exact["raw"] = conv + bias.  Scale / shift form: a power-of-two scale putting the outputs near `target`, a shift in quarter
    steps, an integer residual; exact["conv"] = conv * scale + shift, exact["y"] = that + res."""
    key = (row.name, "exact", seed)
    if key not in _dw_cache:      # (x, w and their conv do not depend on the storage type: once per row)
        _dw_cache.clear()
        g = torch.Generator().manual_seed(seed + 1 + sum(map(ord, row.name)))
        x, w = torch.randint(-8, 9, (row.N, row.C, row.H, row.W), generator=g).double(), torch.randint(-8, 9, (row.Co, row.k, row.k), generator=g).double()
        _dw_cache[key] = (x, w, dw_sums(x, w)[0])
    x, w, acc = _dw_cache[key]
    g = torch.Generator().manual_seed(seed + 2 + sum(map(ord, row.name)))
    Co, k = row.Co, row.k
    o = dict(x=x, w=w, res=None)
    if row.ln:
        o.update(v0=torch.randint(-8000, 8001, (Co,), generator=g).float() * 0.25, v1=torch.rand(Co, generator=g) + 0.5, v2=torch.randn(Co, generator=g) * 0.1)
        exact = {"raw": acc + o["v0"].double().view(1, -1, 1, 1)}
    else:
        p = round(math.log2(target / (24.0 * k)))
        o.update(v0=(2.0 ** (p + torch.randint(0, 2, (Co,), generator=g))).float(), v1=torch.randint(-64, 65, (Co,), generator=g).float() * 0.25, v2=None)
        conv = acc * o["v0"].double().view(1, -1, 1, 1) + o["v1"].double().view(1, -1, 1, 1)
        exact = {"conv": conv, "y": conv}
        if row.res:
            o["res"] = storage(torch.randint(-1000, 1001, tuple(acc.shape), generator=g).double(), dtype)
            exact["y"] = conv + o["res"]
    for e in exact.values():
        assert torch.equal(e.float().double(), e), "the exact result must be an fp32 value"
    return o, exact


def dw_tile_of(row: DwRow, dtype, n, y, x):
    """(tile index in the kernel's walk order, image, tile row, tile column) of output pixel (n, y, x)."""
    th, tw = row.field(dtype, "th"), row.field(dtype, "tw")
    ty, tx = y // th, x // tw
    tiles_x, tiles_y = (row.W + tw - 1) // tw, (row.H + th - 1) // th
    return (n * tiles_y + ty) * tiles_x + tx, n, ty, tx


# ------------------------------------------------------------------------------------------------------------------------------------
# The fused inference kernels: upconv_fused.hip (mtbt_convt2x2_conv3x3_nhwc), node_gemm.hip (mtbt_bifpn_node_nhwc) and mlp_fused.hip
# (mtbt_convnext_mlp_fused_dt / _train); tests/test_gpu_fused_variants.py runs the tables UPCONV_VARIANTS, NODE_VARIANTS, MLP_VARIANTS.
# No term of their own.  Two of the kernels round an INTERMEDIATE to the storage type (the fused map of the node, the hidden activations of
# the MLP) from an fp32 value: the reference rounds the fp64 value at the same point, and where that value lies within the fp32 error of a
# rounding midpoint the kernel may land on the other neighbour (round_flips): such an element may be off by one spacing of the storage
# type, carried to the outputs through the absolute weights of the GEMM behind it.
# ------------------------------------------------------------------------------------------------------------------------------------
def spacing_below(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Distance from |v| (a value of the 16-bit `dtype`, fp64 tensor) down to the next smaller magnitude of `dtype` (at zero: the smallest
    subnormal)."""
    a = v.abs().to(dtype)
    prev = (a.view(torch.int16) - 1).clamp(min=0).view(dtype).double()
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133
    return torch.where(a == 0, torch.full_like(v, tiny), a.double() - prev)


def spacing_above(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Distance from |v| up to the next larger magnitude of `dtype`."""
    return spacing_below(v.abs().to(dtype).view(torch.int16).add(1).view(dtype).double(), dtype)


def round_flips(v: torch.Tensor, dtype: torch.dtype, delta: torch.Tensor):
    """v (fp64) rounded to `dtype`, the elements whose fp32 counterpart (|error| <= delta) may round to the other neighbour, and the width
    such a flip adds (the larger neighbouring spacing, 0 elsewhere)."""
    r = v.to(dtype).double()
    below, above = spacing_below(r, dtype), spacing_above(r, dtype)
    flip = (v - r).abs() >= 0.5 * torch.minimum(below, above) - delta
    return r, flip, flip.double() * torch.maximum(below, above)


# ---- upconv_fused.hip ---------------------------------------------------------------------------------------------------------------
def upconv_sums(x: torch.Tensor, wc: torch.Tensor):
    """(sum, sum of magnitudes) of the composed 2 x 2-tap convolution of include/mtbt_hip.h, NCHW fp64 [N, K, 2H, 2W]: output (2i + a, 2j + b)
    = sum over (rho, sigma, ci) of wc[2a + b][k][rho][sigma][ci] * x[i + a - 1 + rho][j + b - 1 + sigma][ci], zero outside the source map.
    x [N, C, H, W], wc [4, K, 2, 2, C]."""
    (N, C, H, W), K = x.shape, wc.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))                                  # source pixel (r, c) at xp[r + 1][c + 1]
    acc = torch.zeros(N, K, 2 * H, 2 * W, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for a in range(2):
        for b in range(2):
            for rho in range(2):
                for sig in range(2):
                    src = xp[:, :, a + rho:a + rho + H, b + sig:b + sig + W]
                    wt = wc[2 * a + b, :, rho, sig, :]
                    acc[:, :, a::2, b::2] += torch.einsum("kc,nchw->nkhw", wt, src)
                    mag[:, :, a::2, b::2] += torch.einsum("kc,nchw->nkhw", wt.abs(), src.abs())
    return acc, mag


def upconv_shift(shift9: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """shift9 [9, K] as the per-pixel shift [1, K, 2H, 2W]: class rc * 3 + cc, rc / cc = 0 first, 2 last, 1 interior OUTPUT row / column."""
    cls = lambda n: torch.tensor([0] + [1] * (n - 2) + [2])
    idx = cls(2 * H)[:, None] * 3 + cls(2 * W)[None, :]
    return shift9.double()[idx].permute(2, 0, 1).unsqueeze(0)


def upconv_bound(acc, mag, sh, act, out_dtype):
    """act(acc + sh) rounded once; the terms of affine_act_ref with a unit scale and a per-pixel shift.  Returns (ref, bound)."""
    pre = acc + sh
    y = act64(pre, act)
    bnd = ACT_LIPSCHITZ[act] * (ACC * mag + EPI * (pre.abs() + sh.abs())) + act_error(pre, act) + EPI * y.abs()
    return y, bnd + output_rounding(y, out_dtype)


def upconv_ref(x, wc, shift9, act, out_dtype):
    """mtbt_convt2x2_conv3x3_nhwc from the formula of its header: x [N, C, H, W] and wc [4, K, 2, 2, C] in storage precision (the composed
    weights ALREADY rounded), shift9 [9, K] fp32.  Returns (ref, bound, sum of magnitudes), NCHW fp64 [N, K, 2H, 2W]."""
    acc, mag = upconv_sums(x, wc)
    ref, bnd = upconv_bound(acc, mag, upconv_shift(shift9, x.shape[2], x.shape[3]), act, out_dtype)
    return ref, bnd, mag


# Rows: N, H, W, C (16-bit types), K, C32 (the channels of the fp32 run: one slab is 64 bytes, 32 / 16 channels), the activations it runs with,
# the layout and whether the exact-rounding test runs it.  A workgroup owns a 16 x 16 source tile x 128 virtual channels q * K + k (one
# parity q; K = 256: two channel tiles per parity, cbase = 0 / 128); launch: ceil(tiles / 8) slots on each of 8 XCDs, the surplus returns.
#   layout "slice": x = channels 16 .. 16 + C of a C + 32 wide NaN-filled buffer, y = channels 8 .. 8 + K of a K + 16 wide sentinel-filled
#   one, both with a gap of pixel rows after every image (UP_SLICE).
UP_SLICE = dict(xpad=32, xc0=16, xgap=5, ypad=16, yc0=8, ygap=3)


@dataclass(frozen=True)
class UpRow:
    name: str
    N: int
    H: int
    W: int
    C: int               # 0: the row does not run in the 16-bit types
    K: int
    C32: int             # 0: the row does not run in fp32
    acts: Tuple[int, ...] = (ACT_SILU,)
    layout: str = "dense"
    exact: bool = False

    @property
    def dtypes(self):
        return tuple(d for d in DTYPES if self.channels(d))

    def channels(self, dtype):
        return self.C32 if dtype == torch.float32 else self.C

    @property
    def tiles(self):
        return self.N * (self.H // 16) * (self.W // 16)


UPCONV_VARIANTS = [
    UpRow("tile1", 1, 16, 16, 32, 128, 16, acts=(ACT_NONE, ACT_SILU), exact=True),     # one tile: all nine classes in a workgroup; one slab
    UpRow("seam_w", 1, 16, 32, 96, 128, 48),                                           # tile seam in a row; three slabs
    UpRow("seam_h", 1, 32, 16, 96, 128, 48),                                           # tile seam in a column
    UpRow("k256", 2, 16, 16, 64, 256, 64, acts=(ACT_NONE, ACT_SILU), exact=True),      # cbase = 128: two channel tiles per parity
    UpRow("xcd3", 3, 16, 16, 64, 128, 64),                                             # 3 tiles: one slot per XCD, 5 of 8 empty
    UpRow("xcd9", 1, 48, 48, 32, 128, 16),                                             # 9 tiles: two slots per XCD, 7 of 16 empty
    UpRow("model", 1, 16, 16, 256, 256, 0),                                            # the model's channel counts on one tile
    UpRow("slice", 2, 16, 16, 64, 256, 64, layout="slice"),                            # strided x and y, gaps between the images
]
UP_ROWS = {r.name: r for r in UPCONV_VARIANTS}


def up_operands(row: UpRow, dtype, seed=0):
    """Random operands of a row as the kernel reads them: x [N, C, H, W] and wc [4, K, 2, 2, C] in storage precision, shift9 [9, K] fp32 with
    nine different class vectors."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, row.name)))
    C = row.channels(dtype)
    x = storage(torch.randn(row.N, C, row.H, row.W, generator=g), dtype)
    wc = storage(torch.randn(4, row.K, 2, 2, C, generator=g) / (4 * C) ** 0.5, dtype)
    shift9 = torch.randn(9, row.K, generator=g) * 0.3
    return x, wc, shift9


def up_exact_operands(row: UpRow, dtype, seed=0):
    """Integer x and wc in [-8, 8] (exact in every storage type; |sum| <= 64 * 4 C <= 2^16) and a shift9 in steps of 1/64 up to +-64 whose nine
    class vectors differ pairwise: every product, partial sum and the shifted result (at most 17 + 6 bits) is exact in fp32, and a result
    beyond 32 mostly needs rounding in fp16 (11 bits), nearly every one in bf16.  Returns the operands and the exact fp64 result (act none)."""
    g = torch.Generator().manual_seed(seed + 1 + sum(map(ord, row.name)))
    C = row.channels(dtype)
    x = torch.randint(-8, 9, (row.N, C, row.H, row.W), generator=g).double()
    wc = torch.randint(-8, 9, (4, row.K, 2, 2, C), generator=g).double()
    shift9 = torch.randint(-4096, 4097, (9, row.K), generator=g).float() / 64.0
    assert all(not torch.equal(shift9[i], shift9[j]) for i in range(9) for j in range(i))
    exact = upconv_sums(x, wc)[0] + upconv_shift(shift9, row.H, row.W)
    assert torch.equal(exact.float().double(), exact), "the exact result must be an fp32 value"
    return x, wc, shift9, exact


# ---- node_gemm.hip ------------------------------------------------------------------------------------------------------------------
RES_ID, RES_UP_BILINEAR, RES_DOWN_MEAN = 0, 1, 2          # resampling modes of include/mtbt_hip.h that a node takes


def bilinear_up2(x: torch.Tensor, clamp_early: int = 0) -> torch.Tensor:
    """Bilinear x2 with align_corners=False, written out (fp64, NCHW): source coordinate (dst + 1/2) / 2 - 1/2 clamped at 0, the neighbour
    i0 + 1 clamped at the last row / column.  clamp_early: a DEFECT for the sensitivity tests -- the ROW neighbour clamped that many rows
    before the last one."""
    def taps(n_src, early):
        s = ((torch.arange(2 * n_src, dtype=torch.float64) + 0.5) / 2 - 0.5).clamp(min=0)
        i0 = s.floor().long()
        i1 = torch.where(i0 < n_src - 1 - early, i0 + 1, i0)
        return i0, i1, s - i0
    y0, y1, ly = taps(x.shape[2], clamp_early)
    x0, x1, lx = taps(x.shape[3], 0)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    top = (1 - lx) * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def mean2x2(x: torch.Tensor) -> torch.Tensor:
    return 0.25 * (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])


def node_resample(x, mode, clamp_early=0):
    return x if mode == RES_ID else bilinear_up2(x, clamp_early) if mode == RES_UP_BILINEAR else mean2x2(x)


def f32_values(wgts):
    """The fusion weights as the kernel reads them: fp32."""
    return [float(v) for v in torch.tensor(list(wgts), dtype=torch.float32).double()]


def node_fused(inputs, wgts, modes, clamp_early=0):
    """(s, sum of magnitudes) of the fused map s = sum_i wgt_i * resample_i(x_i), fp64 NCHW."""
    wv = f32_values(wgts)
    s = sum(w * node_resample(x, m, clamp_early) for w, x, m in zip(wv, inputs, modes))
    mag = sum(abs(w) * node_resample(x.abs(), m, clamp_early) for w, x, m in zip(wv, inputs, modes))
    return s, mag


def node_output(s, smag, w, shift, act, dtype):
    """act(W round_T(s) + shift) from the exact fused map.  The kernel forms s in fp32: at most 7 roundings of 2^-24 lie on any path from an
    input to s (the bilinear form's two products and two sums, the weight product, two sums of the weighted terms), taken as 4 EPI of the
    summed magnitudes; an element of s within that of a rounding midpoint may be one spacing off (round_flips), which reaches an output
    through |W| and the activation's Lipschitz constant.  Returns (ref, bound, flip mask)."""
    sT, flip, width = round_flips(s, dtype, 4 * EPI * smag)
    w4 = w[:, :, None, None]
    ref, bnd = affine_act_ref(F.conv2d(sT, w4), F.conv2d(sT.abs(), w4.abs()), None, shift, act, None, dtype)
    return ref, bnd + ACT_LIPSCHITZ[act] * F.conv2d(width, w4.abs()), flip


def node_ref(inputs, wgts, modes, w, shift, act, dtype):
    """mtbt_bifpn_node_nhwc: inputs NCHW fp64 in storage precision, wgts the fusion weights, modes the resampling modes, w [K, C] in storage
    precision, shift [K] fp32.  Returns (ref, bound, flip mask of the fused map)."""
    return node_output(*node_fused(inputs, wgts, modes), w, shift, act, dtype)


# Rows: kind "td" (top-down: identity + bilinear x2) on N, H, W = 3, 6, 10 -- 60 pixels per image, so the 64-pixel workgroups 0 .. 2 each span
# two images -- or "out" (output: identity + identity + 2x2 mean) on 2, 5, 7 -- 70 pixels, an odd map, the third input 10 x 14; C = K;
# wdev: the weights come from device memory and wgt[] holds other values; slice: y = channels 8 .. 8 + K of a K + 8 wide sentinel-filled buffer.
NODE_WGT = {"td": (0.55, 0.45), "out": (0.31, 0.42, 0.27)}
NODE_WGT_OTHER = {"td": (0.2, 0.8), "out": (0.5, 0.1, 0.4)}
NODE_MODES = {"td": (RES_ID, RES_UP_BILINEAR), "out": (RES_ID, RES_ID, RES_DOWN_MEAN)}
NODE_SHAPE = {"td": (3, 6, 10), "out": (2, 5, 7)}
NODE_DTYPES = (torch.bfloat16, torch.float16)


@dataclass(frozen=True)
class NodeRow:
    name: str
    kind: str
    C: int
    act: int = ACT_ELU
    wdev: bool = False
    slice: bool = False
    dtypes: Tuple[torch.dtype, ...] = NODE_DTYPES

    @property
    def shape(self):
        return NODE_SHAPE[self.kind]

    @property
    def modes(self):
        return NODE_MODES[self.kind]

    @property
    def pitch(self):
        return self.C + 8 if self.slice else self.C

    @property
    def c0(self):
        return 8 if self.slice else 0


NODE_VARIANTS = [
    NodeRow("td128", "td", 128), NodeRow("td256", "td", 256), NodeRow("out128", "out", 128), NodeRow("out256", "out", 256),
    NodeRow("td256_wdev", "td", 256, wdev=True), NodeRow("out128_wdev", "out", 128, wdev=True),
    NodeRow("td128_slice", "td", 128, slice=True), NodeRow("out256_slice", "out", 256, slice=True),
    NodeRow("td256_none", "td", 256, act=ACT_NONE), NodeRow("out128_none", "out", 128, act=ACT_NONE),
]
NODE_ROWS = {r.name: r for r in NODE_VARIANTS}


def node_operands(row: NodeRow, dtype, seed=0):
    """(inputs NCHW fp64 in storage precision, w [K, C] in storage precision, shift [K] fp32) of a row."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, row.name)))
    N, H, W = row.shape
    sizes = {RES_ID: (H, W), RES_UP_BILINEAR: (H // 2, W // 2), RES_DOWN_MEAN: (2 * H, 2 * W)}
    inputs = [storage(torch.randn(N, row.C, *sizes[m], generator=g), dtype) for m in row.modes]
    w = storage(torch.randn(row.C, row.C, generator=g) / row.C ** 0.5, dtype)
    return inputs, w, torch.randn(row.C, generator=g) * 0.3


def node_row_reference(row: NodeRow, dtype, seed=0):
    """Operands and (ref, bound, flip mask) of a row; the weights that count are NODE_WGT (wdev rows: those in device memory)."""
    inputs, w, shift = node_operands(row, dtype, seed)
    return (inputs, w, shift), node_ref(inputs, NODE_WGT[row.kind], row.modes, w, shift, row.act, dtype)


# ---- mlp_fused.hip ------------------------------------------------------------------------------------------------------------------
def mlp_ref(t, res, w1, b1, w2, b2, dtype, round_h=True):
    """y = res + W2 h + b2, h = round_T(gelu_poly(W1 t + b1)): t [M, D], res [M, D] or None, w1 [4D, D], w2 [D, 4D] in storage precision and
    NATURAL hidden order, b1 / b2 fp32.  The kernel's own polynomial GELU in fp64 (gelu_poly64), not erf + 2.3e-4: a fixed 2.3e-4 on each of
    the 4D hidden units, summed through W2, would be looser than the hidden rounding it has to see.  fc1's fp32 accumulation (ACC of the
    magnitudes) and the fp32 polynomial (half ACT_EVAL) can move a hidden value across a rounding midpoint: round_flips.
    round_h=False: h is NOT rounded (the plain MLP; a defect for the sensitivity tests).
    Returns (ref, bound, pre = W1 t + b1, bound of pre rounded once to T, flip mask of the hidden units)."""
    pre = t @ w1.t() + b1.double()
    pre_err = ACC * (t.abs() @ w1.abs().t() + b1.double().abs())
    h64 = gelu_poly64(pre)
    h, flip, width = round_flips(h64, dtype, ACT_LIPSCHITZ[ACT_GELU_POLY] * pre_err + 0.5 * ACT_EVAL * (1 + h64.abs()))
    if not round_h:
        h = h64
    r = res if res is not None else torch.zeros_like(t)
    ref = r + h @ w2.t() + b2.double()
    bnd = output_rounding(ref, dtype) + ACC * (h.abs() @ w2.abs().t() + r.abs() + b2.double().abs()) + width @ w2.abs().t()
    return ref, bnd, pre, output_rounding(pre, dtype) + pre_err, flip


def mlp_hidden_order():
    """Column order of the inference entry's fc2 weight inside a group of 32 hidden units (include/mtbt_hip.h): slot 8 g + j holds hidden
    4 g + j (j < 4) or 16 + 4 g + (j - 4)."""
    kk = torch.arange(32)
    g, j = kk // 8, kk % 8
    return torch.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4))


def mlp_permute_w2(w2: torch.Tensor) -> torch.Tensor:
    idx = (torch.arange(w2.shape[1] // 32)[:, None] * 32 + mlp_hidden_order()[None, :]).reshape(-1)
    return w2[:, idx].contiguous()


def mlp_train_rows(n4d: int) -> torch.Tensor:
    """Row order of the training entry's fc1 weight / bias (include/mtbt_hip.h): row 16 b + 4 g + e of a group of 32 holds hidden 8 g + 4 b + e."""
    return torch.arange(n4d).view(-1, 4, 2, 4).permute(0, 2, 1, 3).reshape(-1)


# Rows: D, M, res, train.  A workgroup owns 128 pixels, a wave 32 (two 16-pixel fragments).  M = 1: one pixel; 17: less than a fragment pair;
# 33: the second wave holds one pixel; 127 / 129: one workgroup -+ 1; 300: three workgroups.  D = 96 the streaming kernel, 192 the pipelined
# one, 384 the pair kernel; train: the two HP forms (bf16, D = 96 / 192) with the fc1 pre-activation as a second output.
MLP_DTYPES = (torch.bfloat16, torch.float16)


@dataclass(frozen=True)
class MlpRow:
    name: str
    D: int
    M: int
    res: bool = True
    train: bool = False
    dtypes: Tuple[torch.dtype, ...] = MLP_DTYPES


MLP_VARIANTS = ([MlpRow(f"d{D}_m{M}", D, M) for D in (96, 192, 384) for M in (1, 17, 33, 127, 129, 300)]
                + [MlpRow(f"d{D}_m129_nores", D, 129, res=False) for D in (96, 192, 384)]
                + [MlpRow(f"train_d{D}_m{M}", D, M, train=True, dtypes=(torch.bfloat16,)) for D in (96, 192) for M in (17, 129, 300)])
MLP_ROWS = {r.name: r for r in MLP_VARIANTS}


def mlp_operands(row: MlpRow, dtype, seed=0):
    """(t, res or None, w1, b1, w2, b2) of a row: storage precision, natural hidden order, the scales of the fp16 test before the table."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, row.name)))
    D, M = row.D, row.M
    t = storage(torch.randn(M, D, generator=g), dtype)
    res = storage(torch.randn(M, D, generator=g) * 0.1, dtype)
    w1 = storage(torch.randn(4 * D, D, generator=g) / D ** 0.5, dtype)
    w2 = storage(torch.randn(D, 4 * D, generator=g) / (4 * D) ** 0.5, dtype)
    b1, b2 = torch.randn(4 * D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1
    return t, (res if row.res else None), w1, b1, w2, b2


def mlp_row_reference(row: MlpRow, dtype, seed=0):
    o = mlp_operands(row, dtype, seed)
    return o, mlp_ref(*o, dtype)
