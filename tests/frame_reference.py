"""CPU reference of the frame operator (`postprocess.masks_to_frames`): a torch restatement of its contract.  TEST INFRASTRUCTURE.

A frame is (H0, W0, scale), scale = S / max(H0, W0) as the letterbox returns it; `up` = letterboxed pixels per prototype pixel;
step = float32(scale / up) prototype pixels per frame pixel.  Everything below is fp32, one operation at a time:

  boxes   clamp(boxes / float32(scale), 0, (W0, H0, W0, H0)), rows k >= count zero
  logit   sx = max((X + 0.5) * step - 0.5, 0); x0 = min(int(sx), wp-1); x1 = min(x0+1, wp-1); lx = clamp(sx - x0, 0, 1); same for y;
          v = (1-ly)*((1-lx)*low[y0,x0] + lx*low[y0,x1]) + ly*((1-lx)*low[y1,x0] + lx*low[y1,x1]),  low = coeffs @ protos
  bit     v > 0 (and, cropping, x1f <= X < x2f and y1f <= Y < y2f of the frame box)
  packed  rows of 8 * ceil(W0 / 64) bytes, numpy.packbits(bitorder="little"), padding bits zero
"""
import numpy as np
import torch


def frame_step(scale: float, up: float) -> float:
    return float(np.float32(float(scale) / float(up)))


def pitch_of(W0: int) -> int:
    return 8 * ((int(W0) + 63) // 64)


def _taps(n: int, size: int, step: float):
    d = torch.arange(n, dtype=torch.float32)
    s = torch.clamp((d + 0.5) * torch.tensor(step, dtype=torch.float32) - 0.5, min=0)
    i0 = torch.clamp(s.to(torch.int64), max=size - 1)
    i1 = torch.clamp(i0 + 1, max=size - 1)
    l1 = torch.clamp(s - i0.to(torch.float32), 0, 1)
    return i0, i1, 1 - l1, l1


def frame_logits(coeffs: torch.Tensor, protos: torch.Tensor, H0: int, W0: int, scale: float, up: float) -> torch.Tensor:
    """coeffs [K,nm], protos [nm,hp,wp] -> logits [K,H0,W0] at the original image's pixels."""
    nm, hp, wp = protos.shape
    step = frame_step(scale, up)
    low = torch.einsum("kc,chw->khw", coeffs.float(), protos.float())
    y0, y1, b0, b1 = _taps(H0, hp, step)
    x0, x1, a0, a1 = _taps(W0, wp, step)
    top = a0 * low[:, y0][:, :, x0] + a1 * low[:, y0][:, :, x1]
    bot = a0 * low[:, y1][:, :, x0] + a1 * low[:, y1][:, :, x1]
    return b0[:, None] * top + b1[:, None] * bot


def frame_boxes(boxes: torch.Tensor, count: int, H0: int, W0: int, scale: float) -> torch.Tensor:
    """boxes [K,4] letterboxed xyxy -> frame boxes [K,4]; rows k >= count are zeros."""
    out = boxes.float() / torch.tensor(float(scale), dtype=torch.float32)
    hi = torch.tensor([W0, H0, W0, H0], dtype=torch.float32)
    out = torch.minimum(torch.clamp(out, min=0), hi)
    out[count:] = 0
    return out


def crop_region(fboxes: torch.Tensor, H0: int, W0: int) -> torch.Tensor:
    """bool [K,H0,W0]: x1 <= X < x2 and y1 <= Y < y2 (ultralytics crop_mask)."""
    X = torch.arange(W0, dtype=torch.float32)[None, None, :]
    Y = torch.arange(H0, dtype=torch.float32)[None, :, None]
    x1, y1, x2, y2 = (fboxes[:, i, None, None] for i in range(4))
    return (x1 <= X) & (X < x2) & (y1 <= Y) & (Y < y2)


def pack_bits(bits: torch.Tensor) -> torch.Tensor:
    """bool [K,H0,W0] -> uint8 [K,H0,pitch]: pixel X is bit X & 7 of byte X >> 3, padding bits zero."""
    K, H0, W0 = bits.shape
    padded = np.zeros((K, H0, pitch_of(W0) * 8), dtype=np.uint8)
    padded[:, :, :W0] = bits.numpy().astype(np.uint8)
    return torch.from_numpy(np.packbits(padded, axis=-1, bitorder="little"))


def unpack_bits(packed: torch.Tensor, W0: int) -> torch.Tensor:
    """uint8 [K,H0,pitch] -> bool [K,H0,pitch*8] (ALL bits, the padding included; slice [..., :W0] for the image)."""
    return torch.from_numpy(np.unpackbits(packed.cpu().numpy(), axis=-1, bitorder="little")).bool()


def frame_reference(protos, mc, keep_anchor, counts, boxes, frames, up, crop=False):
    """The whole operator for a batch on the CPU.  protos [B,nm,hp,wp]; mc [B,nm,A]; keep_anchor [B,K]; counts [B]; boxes [B,K,4].
    Returns a list of dict(logits [K,H0,W0] (rows >= count zero), bits bool, region bool or None, boxes [K,4], packed uint8)."""
    out = []
    K = keep_anchor.shape[1]
    for b, (H0, W0, scale) in enumerate(frames):
        n = int(counts[b])
        coeffs = torch.zeros(K, mc.shape[1])
        coeffs[:n] = mc[b, :, keep_anchor[b, :n].long()].t()
        logits = frame_logits(coeffs, protos[b], H0, W0, scale, up)
        logits[n:] = 0
        fb = frame_boxes(boxes[b], n, H0, W0, scale)
        bits = logits > 0
        region = None
        if crop:
            region = crop_region(fb, H0, W0)
            bits = bits & region
        out.append({"logits": logits, "bits": bits, "region": region, "boxes": fb, "packed": pack_bits(bits)})
    return out
