"""CPU restatement of `mtbt_seg_to_frames` (include/mtbt_hip.h): the semantic mask in the image frame, views averaged, tiles blended.

Written from the rule, not from the kernel.  numpy float32 arrays: every `+`, `*`, `/` below is one correctly rounded fp32 operation, in the
order the rule writes them.  `dtype=np.float64` evaluates the same rule in double (the tap POSITIONS -- x0, x1, lx -- stay the fp32 ones:
they are part of the rule, not of its rounding).

  L_s[y,x] = (((0 + q[j,0] P_s[y,x,0]) + q[j,1] P_s[y,x,1]) + ... + q[j,31] P_s[y,x,31]) + q[j,32]
  for the sources s ascending whose window holds (X, Y), num = den = 0 at the start:
    (x0, x1, lx) = frame_tap(X, step_s, pox_s, G);  (y0, y1, ly) likewise with poy_s
    U_s[y,x] = L_s[fy(a), fx(b)],  (a,b) = (x,y) if orient bit 2 else (y,x),  fy(a) = G-1-a if bit 1,  fx(b) = G-1-b if bit 0
    tap = (1-ly)*((1-lx)*U[y0,x0] + lx*U[y0,x1]) + ly*((1-lx)*U[y1,x0] + lx*U[y1,x1])
    bx  = blend_s ? (1-lx)*tab[x0] + lx*tab[x1] : 1;  by likewise;  w = weight_s * (bx * by)
    num = num + w * tap;  den = den + w
  v = den > 0 ? num / den : 0;  bit = den > 0 && v > threshold
"""
import ctypes as C

import numpy as np

F = np.float32


def project(P, q, dtype=F):
    """P [G, G, 32] (NHWC), q [33] -> L [G, G]: the serial sum, c ascending, multiply then add, the bias last."""
    P, q = P.astype(dtype), q.astype(dtype)
    acc = np.zeros(P.shape[:2], dtype)
    for c in range(32):
        acc = acc + q[c] * P[:, :, c]
    return acc + q[32]


def frame_tap(d, step, po, size):
    """torch's align_corners=False source index for destination indices d (int array), a grid that starts `po` prototype pixels in."""
    s = (d.astype(F) + F(0.5)) * F(step) - F(0.5) - F(po)
    s = np.where(s > 0, s, F(0)).astype(F)
    i = s.astype(np.int32)
    i0 = np.minimum(i, size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    w = s - i0.astype(F)
    w = np.where(w > 0, w, F(0)).astype(F)
    return i0, i1, np.where(w < 1, w, F(1)).astype(F)


def upright(L, orient):
    G = L.shape[0]
    y, x = np.mgrid[0:G, 0:G]
    a, b = (x, y) if orient & 4 else (y, x)
    return L[G - 1 - a if orient & 2 else a, G - 1 - b if orient & 1 else b]


def blend_frame(H0, W0, sources, tab, threshold, dtype=F):
    """sources: dicts(L [G,G], tile (the mtbt_tile fields), orient, weight, blend), in the rule's order.
    Returns dict(logits [H0,W0], bits bool [H0,W0], den [H0,W0])."""
    num, den = np.zeros((H0, W0), dtype), np.zeros((H0, W0), dtype)
    one = dtype(1)
    for s in sources:
        t, G = s["tile"], s["L"].shape[0]
        U = upright(s["L"].astype(dtype), s["orient"])
        X, Y = np.arange(t["wx0"], t["wx1"]), np.arange(t["wy0"], t["wy1"])
        x0, x1, lx = frame_tap(X, t["step"], t["pox"], G)
        y0, y1, ly = frame_tap(Y, t["step"], t["poy"], G)
        lx, ly = lx.astype(dtype)[None, :], ly.astype(dtype)[:, None]
        r0, r1 = y0[:, None], y1[:, None]
        c0, c1 = x0[None, :], x1[None, :]
        tap = (one - ly) * ((one - lx) * U[r0, c0] + lx * U[r0, c1]) + ly * ((one - lx) * U[r1, c0] + lx * U[r1, c1])
        if s["blend"]:
            tb = tab.astype(dtype)
            bx = (one - lx) * tb[c0] + lx * tb[c1]
            by = (one - ly) * tb[r0] + ly * tb[r1]
        else:
            bx, by = np.ones((1, X.size), dtype), np.ones((Y.size, 1), dtype)
        w = dtype(s["weight"]) * (bx * by)
        win = (slice(t["wy0"], t["wy1"]), slice(t["wx0"], t["wx1"]))
        num[win] = num[win] + w * tap
        den[win] = den[win] + w
    seen = den > 0
    v = np.where(seen, num / np.where(seen, den, one), dtype(0)).astype(dtype)
    return {"logits": v, "bits": seen & (v > dtype(F(threshold))), "den": den}


def full_view(n, H0, W0, scale, up=4.0):
    """The descriptor of a whole-image pass over frame (H0, W0, scale): window = the frame, no offset, the frame's step."""
    return {"image": n, "pox": 0, "poy": 0, "wx0": 0, "wy0": 0, "wx1": W0, "wy1": H0, "height": H0, "width": W0,
            "step": C.c_float(scale / up).value, "scale": C.c_float(scale).value, "fox": 0.0, "foy": 0.0}


def is_whole(t):
    return (t["wx0"], t["wy0"], t["wx1"], t["wy1"]) == (0, 0, t["width"], t["height"])


def seg_reference(passes, projs, frames, orients, weights, tiles=None, tab=None, threshold=0.0, up=4.0, dtype=F):
    """What `postprocess.seg_to_frames` computes.  passes: M arrays [NT, 32, G, G] (logical NCHW); projs: M arrays [33] (32 weights, the
    bias); frames [(H0, W0, scale)]; orients / weights per pass; tiles: `slice_geometry`'s lists or None (one whole-image source per pass).
    The sources of image n: pass m ascending, then tile ascending; the table applies to tile sources, whole-image ones are constant.
    Returns (per image dict of `blend_frame`, low: the projector logits of every source in source order)."""
    out, low, t0 = [], [], 0
    for n, (H0, W0, scale) in enumerate(frames):
        own = [(n, full_view(n, H0, W0, scale, up))] if tiles is None else [(t0 + i, t) for i, t in enumerate(tiles[n])]
        t0 += len(own) if tiles is not None else 0
        sources = []
        for m, P in enumerate(passes):
            for slot, t in own:
                L = project(np.ascontiguousarray(P[slot].transpose(1, 2, 0)), projs[m], dtype)
                low.append(L)
                sources.append({"L": L, "tile": t, "orient": orients[m], "weight": weights[m],
                                "blend": tab is not None and tiles is not None and not is_whole(t)})
        out.append(blend_frame(H0, W0, sources, tab, threshold, dtype))
    return out, low


def pack(bits):
    """bool [H0, W0] -> uint8 [H0, 8 * ceil(W0 / 64)], little-endian bits, zero padding."""
    H0, W0 = bits.shape
    pitch = 8 * ((W0 + 63) // 64)
    out = np.zeros((H0, pitch), np.uint8)
    pk = np.packbits(bits, axis=1, bitorder="little")
    out[:, :pk.shape[1]] = pk
    return out


def inputs(seed, shape):
    """Prototypes ~ N(0, 1) of `shape` and a projector [33] ~ N(0, 1), float32."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(F), rng.standard_normal(33).astype(F)
