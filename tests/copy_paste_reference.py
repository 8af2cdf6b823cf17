"""The copy-paste rule of include/mtbt_hip.h `mtbt_copy_paste`, restated in plain numpy on UNPACKED bool planes and float canvases, written
from the header's statement of the rule and not from the kernel: no words, no funnel shifts, one pixel at a time through index arrays.
`pack` / `unpack` convert to and from the library's bit-packed layout (bit x of a row lives in byte x // 8, bit x % 8; pitch = 8 ceil(S / 64))."""
import numpy as np


def pitch_of(S: int) -> int:
    return 8 * ((S + 63) // 64)


def pack(planes: np.ndarray) -> np.ndarray:
    """bool [M, S, S] -> uint8 [M, S, pitch], padding bits zero."""
    M, S, _ = planes.shape
    wide = np.zeros((M, S, 8 * pitch_of(S)), dtype=bool)
    wide[:, :, :S] = planes
    return np.packbits(wide, axis=2, bitorder="little")


def unpack(packed: np.ndarray, S: int) -> np.ndarray:
    """uint8 [M, S, pitch] -> (bool [M, S, S], True when every padding bit is zero)."""
    bits = np.unpackbits(packed, axis=2, bitorder="little").astype(bool)
    return bits[:, :, :S], not bits[:, :, S:].any()


def canvas_of_row(row_off, r: int) -> int:
    """The canvas whose row_off range holds row r."""
    for j in range(len(row_off) - 1):
        if row_off[j] <= r < row_off[j + 1]:
            return j
    raise ValueError(f"row {r} lies on no canvas")


def translated(plane: np.ndarray, dx: int, dy: int, flip: int):
    """T[y'][x'] = plane[y][x], y = y' - dy, x = flip ? S - 1 - (x' - dx) : x' - dx, 0 outside: -> (T, y, x, inside) with the index grids."""
    S = plane.shape[0]
    yp, xp = np.mgrid[0:S, 0:S]
    y = yp - dy
    x = S - 1 - (xp - dx) if flip else xp - dx
    inside = (x >= 0) & (x < S) & (y >= 0) & (y < S)
    T = np.zeros((S, S), dtype=bool)
    T[inside] = plane[y[inside], x[inside]]
    return T, y, x


def record(plane: np.ndarray):
    """(popcount, [x1, y1, x2, y2] tight with exclusive maxima; zeros when empty)."""
    ys, xs = np.nonzero(plane)
    if len(ys) == 0:
        return 0, [0, 0, 0, 0]
    return len(ys), [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def row_from_box(image, cls, box, S: int) -> np.ndarray:
    x1, y1, x2, y2 = box
    f = np.float32
    return np.array([image, cls, f(x1 + x2) / f(2 * S), f(y1 + y2) / f(2 * S), f(x2 - x1) / f(S), f(y2 - y1) / f(S)], dtype=np.float32)


def copy_paste(images, planes, row_off, rows_in, paste_off, entries):
    """images f32 [B, 3, S, S]; planes bool [M, S, S]; row_off int [B + 1]; rows_in f32 [M, 6]; paste_off int [B + 1]; entries int [P, 8].
    -> dict(images f32 [B,3,S,S], planes bool [M+P,S,S], masks f32 [B,1,S,S], area_before, area uint32 [M+P], box int32 [M+P,4],
    rows f32 [M+P,6])."""
    images = np.asarray(images, dtype=np.float32)
    planes = np.asarray(planes, dtype=bool)
    rows_in = np.asarray(rows_in, dtype=np.float32).reshape(-1, 6)
    entries = np.asarray(entries, dtype=np.int64).reshape(-1, 8)
    B, _, S, _ = images.shape
    M, P = planes.shape[0], entries.shape[0]
    out_images = images.copy()
    out_planes = np.zeros((M + P, S, S), dtype=bool)
    masks = np.zeros((B, 1, S, S), dtype=np.float32)
    area_before, area = np.zeros(M + P, dtype=np.uint32), np.zeros(M + P, dtype=np.uint32)
    box = np.zeros((M + P, 4), dtype=np.int32)
    rows = np.zeros((M + P, 6), dtype=np.float32)
    for i in range(B):
        es = list(range(int(paste_off[i]), int(paste_off[i + 1])))
        T = {}
        for e in es:                                                   # table order: a later entry overwrites an earlier one = lies above it
            r, dx, dy, flip = (int(v) for v in entries[e, :4])
            j = canvas_of_row(row_off, r)
            T[e], y, x = translated(planes[r], dx, dy, flip)
            out_images[i][:, T[e]] = images[j][:, y[T[e]], x[T[e]]]    # from the INPUT: mutual and self-pastes read pristine pixels
        U = np.zeros((S, S), dtype=bool)
        for e in reversed(es):                                         # U is the OR of the later entries when entry e is reached
            out_planes[M + e] = T[e] & ~U
            U |= T[e]
            area_before[M + e] = T[e].sum()
            area[M + e], box[M + e] = record(out_planes[M + e])
            cls = rows_in[int(entries[e, 0]), 1]
            rows[M + e] = row_from_box(np.float32(i), cls, box[M + e], S) if area[M + e] else [i, cls, 0, 0, 0, 0]
        union = U.copy()
        for m in range(int(row_off[i]), int(row_off[i + 1])):
            out_planes[m] = planes[m] & ~U
            union |= planes[m]
            area_before[m] = planes[m].sum()
            area[m], box[m] = record(out_planes[m])
            if area[m] == area_before[m]:
                rows[m] = rows_in[m]
            elif area[m] == 0:
                rows[m] = [rows_in[m, 0], rows_in[m, 1], 0, 0, 0, 0]
            else:
                rows[m] = row_from_box(rows_in[m, 0], rows_in[m, 1], box[m], S)
        masks[i, 0] = union
    return {"images": out_images, "planes": out_planes, "masks": masks, "area_before": area_before, "area": area, "box": box, "rows": rows}
