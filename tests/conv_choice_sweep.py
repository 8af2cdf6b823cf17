"""Canonical record of the conv host dispatch (not a test): what `tests/test_cpu_conv_choice.py` hashes and compares with
`tests/golden/conv_choice.json`.

The query entry points of the convolution family launch nothing and dereference no pointer, so they run without a device on argument
blocks with fake aligned pointers.  For every block of the sweep the record holds
  * `kc`: (rc, choice[0..3]) of mtbt_conv_kernel_choice on the block as it stands;
  * `layout`: (rc, rows, pitch) of mtbt_conv_colsum_layout on the block with a column-sum workspace, without and with squares;
  * `batch`: for 1, 2, 3 and 8 members (copies of the block on buffers of their own), (rc, choice[0..3]) of mtbt_conv_batch_kernel_choice.
The group `batch_refusals` records the batch query (and the n = 0 / 9 / NULL answers of mtbt_conv2d_nhwc_batch, which return before any
launch) on members that differ or overlap.  Output slots the library did not write read -7.

The sweep is deterministic: plain products, thinned by a fixed multiplicative hash of the product index.

Run as a script it prints per group the block count and digest, or the full record of one group, so two libraries can be diffed:
    python tests/conv_choice_sweep.py [--lib path/to/libmtbt_hip.so]
    python tests/conv_choice_sweep.py [--lib ...] hints
    python tests/conv_choice_sweep.py [--lib ...] --fixture        # the fixture's JSON
"""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multitask_bonetumor_yolo_amd import _lib as L  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_choice.json")
QUERIES = ("mtbt_conv_kernel_choice", "mtbt_conv_colsum_layout", "mtbt_conv_batch_kernel_choice", "mtbt_conv2d_nhwc_batch")
UNSET = -7

DTYPES = (L.BF16, L.F16, L.F32)
FORMS = ((1, 1, 0), (2, 2, 0), (3, 1, 1), (3, 2, 1))                   # (k, stride, pad)
MAPS = ((5, 5), (9, 7), (16, 16), (20, 20), (40, 40), (48, 16), (80, 80), (160, 160))
BATCHES = (1, 2, 16, 32)
CS = (64, 96, 128, 192, 256, 384, 768, 3072)
KS = (2, 16, 32, 48, 64, 96, 128, 160, 192, 256, 384, 512, 768)
TILES = tuple((tc, tp) for tp in (128, 64) for tc in (128, 96, 64, 32))
MEMBER_COUNTS = (1, 2, 3, 8)
X0, W0, Y0, SCALE0, SHIFT0, RES0, Y20, WS0, CSUM0 = (k << 40 for k in range(1, 10))     # fake buffers, 1 TiB apart
MEMBER_STEP = 1 << 36                                                   # member j of a batch: every buffer 64 GiB further on


def load(path=None):
    if path is None:
        from multitask_bonetumor_yolo_amd import build as B
        B.build()
        return L.load()
    lib = C.CDLL(path)
    for name in QUERIES:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SYMBOLS[name]
    return lib


def es_of(dtype):
    return 4 if dtype == L.F32 else 2


def block(dtype, N, H, W, Cin, K, form=(1, 1, 0), act=L.ACT_SILU, f32_out=False, scale=True, res=False, y2=False, convt=False,
          policy=0, hint=0, y_slice=0, x_off=0):
    """One mtbt_conv_args as engine.Plan.conv fills it.  `y_slice` > 0: the output is the channel slice at that offset of a K + y_slice wide
    buffer (y_slice = 2: not 16-byte aligned, the scalar epilogue); `x_off`: bytes added to x."""
    k, stride, pad = form
    a = L.ConvArgs()
    out = L.F32 if f32_out else dtype
    oes = es_of(out)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ldy = K + y_slice
    a.x, a.w, a.y, a.shift = X0 + x_off, W0, Y0 + y_slice * oes, SHIFT0
    a.scale, a.res, a.y2 = (SCALE0 if scale else None), (RES0 if res else None), (Y20 + y_slice * oes if y2 else None)
    a.N, a.H, a.W, a.C, a.K, a.R, a.S, a.stride, a.pad, a.Ho, a.Wo = N, H, W, Cin, K, k, k, stride, pad, Ho, Wo
    a.x_pixel_stride, a.x_batch_stride = Cin, H * W * Cin
    a.y_pixel_stride, a.y_batch_stride = ldy, Ho * Wo * ldy
    if convt:
        a.y_pixel_stride, a.y_batch_stride = K // 4, 4 * Ho * Wo * (K // 4)
    a.res_pixel_stride, a.res_batch_stride = (K, Ho * Wo * K) if res else (0, 0)
    a.dtype, a.out_dtype, a.act = dtype, out, act
    a.out_mode = L.OUT_CONVT2X2 if convt else L.OUT_NHWC
    a.tile_hint, a.policy = hint, policy
    return a


def copy_of(a):
    b = L.ConvArgs()
    C.memmove(C.byref(b), C.byref(a), C.sizeof(L.ConvArgs))
    return b


def member(a, j):
    """The block on buffers of its own (alignment of every pointer kept)."""
    b = copy_of(a)
    for f in ("x", "w", "y", "scale", "shift", "res", "y2"):
        if getattr(b, f):
            setattr(b, f, getattr(b, f) + j * MEMBER_STEP)
    return b


def array_of(members):
    arr = (L.ConvArgs * max(len(members), 1))()
    for i, m in enumerate(members):
        C.memmove(C.byref(arr, i * C.sizeof(L.ConvArgs)), C.byref(m), C.sizeof(L.ConvArgs))
    return arr


def fields_of(a):
    return {name: (getattr(a, name) or 0) for name, _ in L.ConvArgs._fields_}


def kernel_choice(lib, a):
    out = (C.c_int32 * 4)(*[UNSET] * 4)
    return [lib.mtbt_conv_kernel_choice(C.byref(a), out)] + list(out)


def colsum_layout(lib, a, squares):
    b = copy_of(a)
    b.colsum_ws, b.colsum_ws_bytes, b.colsum_sq = WS0, 1 << 40, squares
    rows, pitch = C.c_int64(UNSET), C.c_int32(UNSET)
    return [lib.mtbt_conv_colsum_layout(C.byref(b), C.byref(rows), C.byref(pitch)), rows.value, pitch.value]


def batch_choice(lib, members, n=None):
    out = (C.c_int32 * 4)(*[UNSET] * 4)
    return [lib.mtbt_conv_batch_kernel_choice(array_of(members), len(members) if n is None else n, out)] + list(out)


def record(lib, a):
    return {"args": fields_of(a), "kc": kernel_choice(lib, a), "layout": [colsum_layout(lib, a, 0), colsum_layout(lib, a, 1)],
            "batch": {str(n): batch_choice(lib, [member(a, j) for j in range(n)]) for n in MEMBER_COUNTS}}


def thinned(product, one_in):
    """Every element of `product` whose index hashes into the first of `one_in` buckets (Knuth's multiplicative hash: no stride that
    could fall in step with an axis of the product)."""
    for i, item in enumerate(product):
        if one_in == 1 or (((i * 2654435761) & 0xffffffff) >> 12) % one_in == 0:
            yield item


# ---- the groups --------------------------------------------------------------------------------------------------------------------
def g_tile_rules():
    """The tile heuristics on the whole shape grid: every dtype, form, map, batch, C and K (one in 16 of the product)."""
    for dt, form, (H, W), N, Cin, K in thinned(itertools.product(DTYPES, FORMS, MAPS, BATCHES, CS, KS), 16):
        yield block(dt, N, H, W, Cin, K, form)


def g_thresholds():
    """Workgroup counts one below, at and one above every count the tile rules compare with: maps of g rows of 128 (or 64) output pixels,
    so that a call has exactly g pixel tiles (times the channel tiles of K)."""
    for dt, T, d in itertools.product((L.BF16, L.F32), (256, 300, 512, 1024, 3000, 4096), (-1, 0, 1)):
        g = T + d
        for K, act, W in itertools.product((128, 256, 384), (L.ACT_SILU, L.ACT_ELU), (128, 64)):
            yield block(dt, 1, g, W, 256, K, FORMS[0], act=act)
        for K, W, form in itertools.product((64, 128, 192), (256, 128), (FORMS[1], FORMS[3])):
            yield block(dt, 1, 2 * g, W, 128, K, form)
        for H in (170, 171, 186, 187):                                 # K = 320 (3 channel tiles, 5 x 64): 64-pixel tile count 3 H around 512
            yield block(dt, 1, H, 64, 256, 320, FORMS[0])
        for pol in (0x100 | 0xfe, 0x100 | 0xfd):                       # the round-1 baseline rule: policy bit 0 / bit 1 cleared
            yield block(dt, 1, g, 128, 256, 128, FORMS[0], policy=pol)
            yield block(dt, 1, 2 * g, 256, 128, 128, FORMS[1], policy=pol)


def g_fp32_out():
    """fp32 outputs, bias only and with a scale: the heads' output convs (streaming kernel below 64 outputs) -- one in 6."""
    for dt, form, (H, W), N, Cin, K, scale in thinned(itertools.product(DTYPES, (FORMS[0], FORMS[2]), MAPS, (1, 16), (64, 256, 768), KS, (False, True)), 6):
        yield block(dt, N, H, W, Cin, K, form, act=L.ACT_NONE, f32_out=True, scale=scale)


EPILOGUE_SHAPES = ((16, 40, 40, 256, 256, FORMS[0]), (2, 16, 16, 128, 128, FORMS[2]), (1, 9, 7, 64, 48, FORMS[2]), (16, 80, 80, 128, 128, FORMS[0]),
                   (16, 80, 80, 256, 256, FORMS[0]), (2, 20, 20, 192, 96, FORMS[3]))


def g_epilogue():
    """Activation, scale, residual, second output."""
    acts = ((L.ACT_NONE, None), (L.ACT_SILU, None), (L.ACT_ELU, None), (L.ACT_DGELU_POLY, True))
    for dt, (N, H, W, Cin, K, form), (act, needs_res), scale, res, y2 in itertools.product(DTYPES, EPILOGUE_SHAPES, acts, (True, False), (True, False), (False, True)):
        yield block(dt, N, H, W, Cin, K, form, act=act, scale=scale, res=bool(needs_res or res), y2=y2)


def g_convt():
    """ConvTranspose2d(2, 2) output mode; K % 4 both ways, K / 4 % 8 both ways."""
    for dt, (H, W), N, Cin, K in itertools.product(DTYPES, ((5, 5), (20, 20), (40, 40)), (2, 16), (64, 256), (2, 6, 16, 64, 96, 128, 160, 256)):
        yield block(dt, N, H, W, Cin, K, act=L.ACT_NONE, scale=False, convt=True)


POLICY_SHAPES = ((16, 80, 80, 96, 384, FORMS[0], False), (16, 40, 40, 256, 256, FORMS[0], False), (32, 160, 160, 96, 384, FORMS[0], False),
                 (16, 20, 20, 384, 384, FORMS[0], False), (16, 80, 80, 256, 2, FORMS[0], True), (16, 80, 80, 256, 64, FORMS[0], True),
                 (16, 80, 80, 64, 64, FORMS[2], False), (16, 40, 40, 192, 192, FORMS[2], False), (2, 16, 16, 128, 96, FORMS[2], False),
                 (16, 20, 20, 384, 384, FORMS[2], False), (16, 48, 16, 128, 128, FORMS[2], False), (16, 40, 40, 192, 384, FORMS[3], False),
                 (2, 9, 7, 64, 160, FORMS[2], False), (16, 40, 40, 96, 192, FORMS[1], False))
POLICIES = (0,) + tuple(0x100 | (1 << b) for b in range(8)) + tuple(0x100 | (0xff & ~(1 << b)) for b in range(8)) + (0x100, 0x1ff)


def g_policy():
    """The default policy, and 0x100 | each single policy bit set and cleared."""
    for dt, (N, H, W, Cin, K, form, f32), pol in itertools.product(DTYPES, POLICY_SHAPES, POLICIES):
        yield block(dt, N, H, W, Cin, K, form, act=L.ACT_NONE if f32 else L.ACT_SILU, f32_out=f32, scale=not f32, policy=pol)


HINTS = (0,) + tuple((tc << 16) | tp | (nar << 27) for tc, tp in TILES for nar in (0, 1)) + (
    1 << 25, 1 << 26, (1 << 25) | (1 << 26), 3 << 28, 7 << 28, (2 << 28) | (64 << 16) | 64, (4 << 28) | (1 << 27) | (128 << 16) | 128,
    (48 << 16) | 64, (64 << 16) | 32, 64 << 16, 128)                 # ... stage bits alone and on a tile; tiles no kernel exists for; half a tile
HINT_SHAPES = ((2, 9, 7, 64, 136, FORMS[0], False), (16, 40, 40, 256, 256, FORMS[0], False), (16, 80, 80, 256, 2, FORMS[0], True),
               (1, 16, 16, 64, 48, FORMS[2], False), (16, 80, 80, 128, 128, FORMS[2], False), (16, 20, 20, 96, 96, FORMS[2], False),
               (2, 20, 20, 192, 192, FORMS[3], False), (16, 40, 40, 96, 192, FORMS[1], False))


def g_hints():
    """Hint 0, every table tile with wide and narrow K-steps, bits 25 and 26, the ignored stage bits 28..30, tiles outside the table."""
    for dt, (N, H, W, Cin, K, form, f32), h in itertools.product(DTYPES, HINT_SHAPES, HINTS):
        yield block(dt, N, H, W, Cin, K, form, act=L.ACT_NONE if f32 else L.ACT_SILU, f32_out=f32, scale=not f32, hint=h)


def g_alignment():
    """The scalar epilogue (output slice at channel 2), aligned slices, a misaligned x (MTBT_EALIGN), strides off the 16-byte grid."""
    for dt, (N, H, W, Cin, K, form, f32) in itertools.product(DTYPES, POLICY_SHAPES):
        for kw in (dict(y_slice=2), dict(y_slice=8), dict(y_slice=2, res=True), dict(x_off=2), dict(x_off=8), dict(x_off=2, y_slice=2)):
            yield block(dt, N, H, W, Cin, K, form, act=L.ACT_NONE, f32_out=f32, **kw)
        for f, v in (("x_pixel_stride", Cin + 2), ("x_batch_stride", H * W * Cin + 2), ("res", RES0 + 2), ("y2", Y20 + 4), ("y_batch_stride", 3)):
            a = block(dt, N, H, W, Cin, K, form, res=True, y2=True)
            setattr(a, f, v)
            yield a


def g_refusals():
    """Every documented refusal of one call, and pairs of faults (the first check in the library's order answers)."""
    for dt in DTYPES:
        ok = lambda **kw: block(dt, 2, 20, 20, 128, 128, FORMS[2], **kw)
        yield ok()
        for Cin in (16, 40, 48, 80):                                   # C % (64 bytes / element size)
            yield block(dt, 2, 20, 20, Cin, 128, FORMS[0])
        for f, v in (("Ho", 19), ("Wo", 21), ("act", 9), ("act", -1), ("act", L.ACT_DSILU), ("act", L.ACT_DGELU), ("colsum", CSUM0), ("x", None),
                     ("w", None), ("y", None), ("dtype", 3), ("out_dtype", 3), ("out_dtype", L.BF16 if dt != L.BF16 else L.F16), ("N", 0), ("K", 0),
                     ("stride", 0), ("pad", -1), ("out_mode", 2), ("x_pixel_stride", 64), ("R", 6), ("x_batch_stride", 1 << 30), ("N", 1 << 22)):
            a = ok()
            setattr(a, f, v)
            if f == "R":
                a.S, a.pad, a.Ho, a.Wo = 6, 0, 15, 15
            yield a
        for faults in ((("x", X0 + 2), ("Ho", 19)), (("x", X0 + 2), ("x_pixel_stride", 64)), (("act", 9), ("C", 40)), (("colsum", CSUM0), ("x", X0 + 2)),
                       (("y2", Y20 + 2), ("x", X0 + 2)), (("out_mode", L.OUT_CONVT2X2), ("K", 130))):
            a = ok()
            for f, v in faults:
                setattr(a, f, v)
            yield a
        # TC == 96 with column sums: the rules avoid the tile (no96), a hint that insists is refused
        for K, h in ((96, 0), (192, 0), (96, (96 << 16) | 128), (192, (96 << 16) | 64), (96, (96 << 16) | 64 | (1 << 27))):
            yield block(dt, 16, 40, 40, 128, K, FORMS[0], hint=h)


def batch_refusal_records(lib):
    """Batches whose members differ or overlap, and the member counts outside 1..8."""
    recs = []

    def slices(dt, n=2, K=64, Cin=64, form=FORMS[2], N=2, H=20, **kw):
        ms = []
        for j in range(n):
            a = block(dt, N, H, H, Cin, K, form, **kw)
            a.x, a.y = X0 + j * Cin * es_of(dt), Y0 + j * K * es_of(dt)
            a.x_pixel_stride, a.x_batch_stride, a.y_pixel_stride, a.y_batch_stride = n * Cin, H * H * n * Cin, n * K, H * H * n * K
            ms.append(a)
        return ms

    def add(what, ms, n=None):
        recs.append({"what": what, "members": [fields_of(m) for m in ms], "n": len(ms) if n is None else n, "batch": batch_choice(lib, ms, n)})

    for dt in DTYPES:
        add("ok", slices(dt))
        for n in (0, 9, -1):
            ms = slices(dt, 8) + slices(dt, 1)
            recs.append({"what": f"n = {n}", "batch": batch_choice(lib, ms, n), "launch": lib.mtbt_conv2d_nhwc_batch(array_of(ms), n, None)})
        out = (C.c_int32 * 4)(*[UNSET] * 4)
        recs.append({"what": "NULL", "batch": [lib.mtbt_conv_batch_kernel_choice(None, 1, out)], "launch": lib.mtbt_conv2d_nhwc_batch(None, 1, None),
                     "no choice": lib.mtbt_conv_batch_kernel_choice(array_of(slices(dt)), 2, None)})
        for f, v in (("K", 32), ("C", 128), ("H", 24), ("act", L.ACT_NONE), ("out_dtype", L.F32), ("dtype", (dt + 1) % 3), ("tile_hint", (64 << 16) | 64),
                     ("policy", 0x100 | 7 | 64), ("stride", 2), ("pad", 0), ("R", 1), ("N", 1), ("Ho", 19), ("debug", 1), ("scale", None), ("shift", None),
                     ("res", RES0), ("y2", Y20), ("colsum", CSUM0), ("colsum_ws", WS0), ("colsum_sq", 1), ("x", X0 + 2), ("y", Y0 + 2)):
            for who in (0, 1):
                ms = slices(dt)
                setattr(ms[who], f, v)
                add(f"member {who}: {f}", ms)
        ms = slices(dt)
        ms[1].y = ms[0].y
        add("same output", ms)
        ms = slices(dt)
        ms[1].y = ms[0].y + 64 * es_of(dt) - 16
        add("slices meet", ms)
        ms = slices(dt, 3)
        ms[2].y = ms[0].y
        add("third member on the first", ms)
        dense = [block(dt, 2, 20, 20, 64, 64, FORMS[2]) for _ in range(2)]
        dense[1].y = Y0 + 2 * 400 * 64 * es_of(dt) - 64
        add("dense outputs meet", dense)
        dense[1].y = Y0 + 2 * 400 * 64 * es_of(dt)
        add("dense outputs back to back", dense)
        for h in ((96 << 16) | 64, (64 << 16) | 128, (64 << 16) | 64 | (1 << 27), (48 << 16) | 64):      # tiles the batched kernels do not exist for
            add(f"hint {h:#x}", [member(block(dt, 2, 20, 20, 64, 96, hint=h), j) for j in range(2)])
        add("direct at 128 channels", slices(dt, K=128))
        add("direct at 64 channels by policy", slices(dt, K=128, policy=0x100 | 7 | 32))
        add("first formulation", slices(dt, policy=0x100 | 7 | 16))
        add("ConvT", slices(dt, convt=True, form=FORMS[0]))
    return recs


GROUPS = {"tile_rules": g_tile_rules, "thresholds": g_thresholds, "fp32_out": g_fp32_out, "epilogue": g_epilogue, "convt": g_convt, "policy": g_policy, "hints": g_hints,
          "alignment": g_alignment, "refusals": g_refusals}
ALL_GROUPS = tuple(GROUPS) + ("batch_refusals",)


def group_records(lib, name):
    if name == "batch_refusals":
        return batch_refusal_records(lib)
    return [record(lib, a) for a in GROUPS[name]()]


def digest(records) -> str:
    return hashlib.sha256(json.dumps(records, sort_keys=True).encode()).hexdigest()


def short(rec):
    """A record without its argument block, for the fixture's readable rows."""
    return {k: v for k, v in rec.items() if k not in ("args", "members")}


def group_entry(lib, name, rows=2):
    recs = group_records(lib, name)
    return {"blocks": len(recs), "sha256": digest(recs), "first": [short(r) for r in recs[:rows]]}


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = None
    if "--lib" in argv:
        i = argv.index("--lib")
        path = argv[i + 1]
        del argv[i:i + 2]
    lib = load(path)
    if argv == ["--fixture"]:
        entries = []
        for g in ALL_GROUPS:
            e = group_entry(lib, g)
            rows = ",\n".join("   " + json.dumps(r, sort_keys=True) for r in e["first"])
            entries.append(f' "{g}": {{"blocks": {e["blocks"]}, "sha256": "{e["sha256"]}", "first": [\n{rows}]}}')
        print("{\n" + ",\n".join(entries) + "\n}")
    elif argv:
        json.dump(group_records(lib, argv[0]), sys.stdout, indent=1, sort_keys=True)
        print()
    else:
        for g in ALL_GROUPS:
            e = group_entry(lib, g)
            print(f"{g:16s} {e['blocks']:5d} {e['sha256']}")
