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
  * a fixed term only where an approximation is documented: the polynomial GELU (ACT_GELU_POLY, common.h gelu_poly) has |err| <= 2.3e-4.
"""
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

# activation codes of include/mtbt_hip.h (MTBT_ACT_*)
ACT_NONE, ACT_SILU, ACT_ELU, ACT_GELU, ACT_GELU_POLY = 0, 1, 2, 3, 4
GELU_POLY_ERR = 2.3e-4
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


def gelu_poly64(x: torch.Tensor) -> torch.Tensor:
    """common.h gelu_poly in fp64, from the same fp32 coefficients: x * (1/2 + xc P(xc^2)), xc = clamp(x, -4, 4)."""
    c = [float(torch.tensor(v, dtype=torch.float32)) for v in
         (2.1609857e-08, -1.5335673e-06, 4.6542096e-05, -7.9887325e-04, 8.6900834e-03, -6.4366050e-02, 3.9770728e-01)]
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
