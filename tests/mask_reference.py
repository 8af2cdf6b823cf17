"""numpy side of the instance-mask mAP tests: packing, pixel-count tables and the mask case set, feeding the plain-loop restatement
`coco_reference.coco_loop_iou`.  TEST INFRASTRUCTURE: a plain module (no fixtures) that shares no code with the product.

Every count is an exact integer and every IoU a quotient of exact integers in fp64 -- the device path must reproduce them bit for bit."""
import numpy as np


def pitch_of(W: int) -> int:
    return 8 * ((int(W) + 63) // 64)


def pack_np(bits: np.ndarray) -> np.ndarray:
    """bool [n,H,W] -> uint8 [n,H,pitch]: pixel X is bit X & 7 of byte X >> 3, padding bits zero."""
    n, H, W = bits.shape
    padded = np.zeros((n, H, pitch_of(W) * 8), np.uint8)
    padded[:, :, :W] = bits
    return np.packbits(padded, axis=-1, bitorder="little")


def unpack_np(packed: np.ndarray, W: int) -> np.ndarray:
    return np.unpackbits(packed, axis=-1, bitorder="little")[:, :, :W].astype(bool)


def pair_counts_np(det: np.ndarray, gt: np.ndarray):
    """det bool [K,H,W], gt bool [G,H,W] -> (inter [G,K], det_area [K], gt_area [G]) int64."""
    px = int(np.prod(det.shape[1:]))
    d, g = det.reshape(len(det), px).astype(np.int64), gt.reshape(len(gt), px).astype(np.int64)
    return g @ d.T, d.sum(1), g.sum(1)


def loop_image(scores, labels, det, gt_labels, gt):
    """One image of `coco_loop_iou` from masks: IoU = inter / (det + gt - inter) in fp64 from the integers, 0 for an empty union."""
    inter, da, ga = pair_counts_np(det, gt)
    iou = [[(float(inter[g, d]) / float(da[d] + ga[g] - inter[g, d])) if da[d] + ga[g] - inter[g, d] > 0 else 0.0 for g in range(len(gt))]
           for d in range(len(det))]
    return ([float(s) for s in scores], [int(l) for l in labels], [float(a) for a in da], [int(l) for l in gt_labels], [float(a) for a in ga], iou)


# ---- the case set ---------------------------------------------------------------------------------------------------------------
def _draw(shapes, H, W, dx=0.0, dy=0.0, grow=0.0):
    """Union of rectangles ("r", x, y, w, h) and discs ("d", cx, cy, r), shifted by (dx, dy) and grown by `grow` pixels per side."""
    Y, X = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for s in shapes:
        if s[0] == "r":
            _, x, y, w, h = s
            m |= (X >= x + dx - grow) & (X < x + dx + w + grow) & (Y >= y + dy - grow) & (Y < y + dy + h + grow)
        else:
            _, cx, cy, r = s
            m |= (X - (cx + dx)) ** 2 + (Y - (cy + dy)) ** 2 <= (r + grow) ** 2
    return m


def _random_shapes(rng, H, W):
    size = float(rng.choice([10, 18, 26, 40, 60, 85, 110]))
    shapes = []
    for _ in range(int(rng.integers(1, 3))):
        if rng.uniform() < 0.5:
            w, h = np.minimum(size * rng.uniform(0.7, 1.3, 2), (W - 2, H - 2))
            shapes.append(("r", rng.uniform(0, W - w), rng.uniform(0, H - h), w, h))
        else:
            r = min(size / 2 * rng.uniform(0.8, 1.2), H / 2 - 2)
            shapes.append(("d", rng.uniform(r, W - r), rng.uniform(r, H - r), r))
    return shapes


def mask_case(seed: int, n_img: int = 40, H: int = 128, W: int = 160, K: int = 12):
    """-> per image dict(det bool [K,H,W] (slots >= count are all ones: they must not be read), scores [K], labels [K], count,
    gt bool [G,H,W], gt_labels [G]).  3 classes (class 2: detections only), G = 0 .. 6, images without GT and images without
    detections, counts < K, scores rounded to 0.1 (ties); detections are shifted / grown copies of GT masks so that IoUs spread over
    0.5 .. 0.95.  Planted: image 0 masks of exactly 32^2 and 96^2 pixels; image 1 two identical GT masks; image 2 an empty detection
    against an empty GT mask."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_img):
        G = 0 if i % 9 == 4 else int(rng.integers(1, 6 if i in (1, 2) else 7))      # the planted images add one GT mask
        shapes = [_random_shapes(rng, H, W) for _ in range(G)]
        gl = rng.integers(0, 2, G)
        if i == 0:
            G, shapes, gl = 2, [[("r", 3.0, 5.0, 32.0, 32.0)], [("r", 50.0, 20.0, 96.0, 96.0)]], np.array([0, 1])
        gt = np.stack([_draw(s, H, W) for s in shapes]) if G else np.zeros((0, H, W), bool)
        if i == 1:
            shapes, gl = shapes + [shapes[0]], np.append(gl, gl[0])
            gt = np.concatenate([gt, gt[:1]])
            G += 1
        D = 0 if i % 9 == 7 else int(rng.integers(1, K + 1))
        if i in (0, 1, 2):
            D = max(D, 4)
        det, dl = np.zeros((K, H, W), bool), rng.integers(0, 3, K)
        for d in range(D):
            if G and rng.uniform() < 0.8:
                src = int(rng.integers(0, G))
                sd = float(rng.choice([0.0, 1.0, 3.0, 6.0]))
                det[d] = _draw(shapes[src], H, W, rng.normal(0, sd), rng.normal(0, sd), float(rng.choice([0.0, 0.0, 1.0, -1.0, 3.0])))
                if rng.uniform() < 0.85:
                    dl[d] = gl[src]
            else:
                det[d] = _draw(_random_shapes(rng, H, W), H, W)
        if i == 0:                                                      # exact copies: areas of exactly 1024 and 9216 pixels, IoU 1
            det[0], det[1], dl[0], dl[1] = gt[0], gt[1], 0, 1
        if i == 1:                                                      # det 0 ties on the two identical GT masks; det 1 is one of them
            det[0], det[1], dl[0], dl[1] = _draw(shapes[0], H, W, 1.0, 0.0), gt[0], gl[0], gl[0]
        if i == 2:                                                      # union 0 -> IoU 0: an unmatched detection and a missed GT
            gt = np.concatenate([gt, np.zeros((1, H, W), bool)])
            gl = np.append(gl, 0)
            det[0], dl[0] = False, 0
        det[D:] = True
        scores = np.round(rng.uniform(0, 1, K), 1).astype(np.float32)
        out.append(dict(det=det, scores=scores, labels=dl.astype(np.int64), count=D, gt=gt, gt_labels=np.asarray(gl, np.int64)))
    assert out[0]["gt"][0].sum() == 1024 and out[0]["gt"][1].sum() == 9216
    return out


def loop_images(case):
    return [loop_image(c["scores"][:c["count"]], c["labels"][:c["count"]], c["det"][:c["count"]], c["gt_labels"], c["gt"]) for c in case]
