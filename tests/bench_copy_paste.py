#!/usr/bin/env python3
"""Time the copy-paste augmentation (mtbt_copy_paste) beside `out.copy_()` of the same canvases and planes on the same stream, in one process,
alternating the two.  The copy is the floor: the kernel reads and writes those bytes once, plus the canvas mask it writes and the donor
pixels of the pasted area.  B canvases of S^2 with three blob planes each and two pastes per canvas from the next canvas, one of them
mirrored.  usage: python tests/bench_copy_paste.py [B] [S] [repeats]"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import _lib as L, preprocess as P
B, S, REP = (int(v) for v in (sys.argv[1:4] + ["32", "640", "5"][len(sys.argv) - 1:]))
ROWS, PASTES = 3, 2


def timed(fn, iters=50):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


rng = np.random.default_rng(0)
pitch = 8 * ((S + 63) // 64)
yy, xx = np.mgrid[0:S, 0:S]
blobs = np.zeros((B * ROWS, S, 8 * pitch), dtype=bool)
for m in range(B * ROWS):                                             # lesions of about S / 8 .. S / 5 across
    cx, cy, rx, ry = rng.integers(S // 4, 3 * S // 4), rng.integers(S // 4, 3 * S // 4), rng.integers(S // 16, S // 10), rng.integers(S // 16, S // 10)
    blobs[m, :, :S] = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
planes = torch.from_numpy(np.packbits(blobs, axis=2, bitorder="little")).cuda()
imgs = torch.rand(B, 3, S, S, device="cuda")
rows = torch.zeros(B * ROWS, 6, device="cuda")
rows[:, 0] = torch.arange(B * ROWS, device="cuda") // ROWS
row_off = np.arange(B + 1, dtype=np.int32) * ROWS
paste_off = np.arange(B + 1, dtype=np.int32) * PASTES
entries = np.zeros((B * PASTES, 8), dtype=np.int32)
for i in range(B):
    donor = (i + 1) % B
    entries[PASTES * i] = [donor * ROWS, int(rng.integers(-S // 8, S // 8)), int(rng.integers(-S // 8, S // 8)), 0, 0, 0, 0, 0]
    entries[PASTES * i + 1] = [donor * ROWS + 1, int(rng.integers(-S // 8, S // 8)), int(rng.integers(-S // 8, S // 8)), 1, 0, 0, 0, 0]
out_i, out_p = torch.empty_like(imgs), torch.empty_like(planes)


def plain_copy():
    out_i.copy_(imgs)
    out_p.copy_(planes)


# the entry point alone, into buffers allocated once: what the stream sees without the wrapper's allocations
N = B * (ROWS + PASTES)
o_planes, o_mask, o_rows = torch.empty(N, S, pitch, device="cuda", dtype=torch.uint8), torch.empty(B, 1, S, S, device="cuda"), torch.empty(N, 6, device="cuda")
o_before, o_area, o_box = (torch.empty(N, k, device="cuda", dtype=torch.int32) for k in (1, 1, 4))
I32P = C.POINTER(C.c_int32)
a = L.CopyPasteArgs()
a.images, a.planes, a.rows_in = imgs.data_ptr(), planes.data_ptr(), rows.data_ptr()
a.row_off, a.paste_off, a.entries = row_off.ctypes.data_as(I32P), paste_off.ctypes.data_as(I32P), entries.ctypes.data_as(I32P)
a.out_images, a.out_planes, a.out_masks, a.rows_out = out_i.data_ptr(), o_planes.data_ptr(), o_mask.data_ptr(), o_rows.data_ptr()
a.area_before, a.area, a.box = o_before.data_ptr(), o_area.data_ptr(), o_box.data_ptr()
a.B, a.M, a.P, a.S, a.pitch, a.entry_stride = B, B * ROWS, B * PASTES, S, pitch, 8
lib, stream = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def entry_point():
    L.check(lib.mtbt_copy_paste(C.byref(a), stream), "mtbt_copy_paste")


runs = {"copy_() of canvases + planes": plain_copy,
        "mtbt_copy_paste (buffers kept)": entry_point,
        "copy_paste_batch": lambda: P.copy_paste_batch(imgs, planes, row_off, rows, (paste_off, entries)),
        "copy_paste_batch masks=False": lambda: P.copy_paste_batch(imgs, planes, row_off, rows, (paste_off, entries), masks=False)}
for fn in runs.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
inst = P.copy_paste_batch(imgs, planes, row_off, rows, (paste_off, entries))[3]
pasted_px = int(inst["area"][B * ROWS:].sum())
us = {k: [] for k in runs}
for _ in range(REP):                                                  # alternate, so that drift hits all alike
    for k, fn in runs.items():
        us[k].append(timed(fn))
copy_mb = 2 * (imgs.numel() * 4 + planes.numel()) / 1e6
base = min(us["copy_() of canvases + planes"])
print(f"B={B} S={S}: {ROWS} planes and {PASTES} pastes a canvas, {pasted_px / B:.0f} pasted px a canvas; the copy moves {copy_mb:.0f} MB (read + write)")
for k, v in us.items():
    print(f"{k:30s} best {min(v):8.1f} us  median {sorted(v)[len(v) // 2]:8.1f} us  spread {max(v) - min(v):6.1f} us  x{min(v) / base:.2f} of the copy", flush=True)
