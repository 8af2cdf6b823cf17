"""Sliced inference: large images are cut into overlapping S x S tiles at or near native resolution, plus the whole image once, and the
per-tile results are merged in the image's own pixel frame on the device (SAHI-style; the reference has no counterpart).

    from multitask_bonetumor_yolo_amd import detect_sliced
    out = detect_sliced(model, raw_images, 640, masks="vote", crop=True)        # raw BGR uint8 [H0, W0, 3] CUDA tensors, any sizes
    mask_map.update_batched(out, gt_masks, gt_labels)                            # boxes_frame / masks_frame / scores / labels / counts

`slice_geometry` -> `slice_batch` (`mtbt_augment_batch` draws each tile) -> `model(x, "infer")` + `detect_and_segment` in chunks of
`batch` tiles -> `merge_tiles` (`mtbt_merge_tiles`) -> `vote_tile_masks` (`mtbt_vote_tile_masks`).  The only host work is the tile
geometry; nothing synchronises with the device.
"""
from typing import Sequence

import torch

from .postprocess import CONF_TH, NMS_IOU, TOP_K, detect_and_segment, merge_tiles, seg_to_frames, vote_tile_masks
from .preprocess import slice_batch, slice_geometry


@torch.no_grad()
def detect_sliced(model, raw_images: Sequence[torch.Tensor], img_size: int, *, zoom: float = 1.0, overlap: float = 0.2,
                  full_view: bool = True, batch: int = 16, conf_th: float = CONF_TH, iou_th: float = NMS_IOU, tile_top_k: int = TOP_K,
                  metric: str = "ios", thr: float = 0.5, skip_thr: float = 0.0, top_k: int = TOP_K, class_agnostic: bool = False,
                  masks=False, crop: bool = False, semantic=None, blend="gaussian", seg_threshold: float = 0.0):
    """Detections (and instance masks) of raw images of any sizes, in their own pixel coordinates.

    `raw_images`: decoded BGR uint8 [H0, W0, 3] CUDA tensors.  Each is cut by `slice_geometry(sizes, img_size, zoom, overlap, full_view)`
    (at most 64 tiles per image and 64 * tile_top_k <= 4096 slots); the model sees the tiles `batch` at a time; conf_th / iou_th /
    tile_top_k are each tile's NMS, metric / thr / skip_thr / top_k / class_agnostic the merge (`postprocess.merge_tiles`).

    Returns `merge_tiles`' dict: boxes_frame [N,top_k,4] in image pixels (also "boxes"), scores, labels, counts, n_members, lead_tile,
    lead_slot, lead_anchor, member_slot, n_left, tiles.  `masks="vote"` adds `masks_frame` (bit-packed uint8 [top_k, H0_n, pitch_n] per
    image, cropped to the merged boxes with `crop`) and `vote_coeff` (`postprocess.vote_tile_masks`); the result then feeds
    `DeviceMaskMeanAveragePrecision.update_batched` as it is.

    `semantic` (the trainer's `seg_proto_projector`: an nn.Conv2d(32, 1, 1) or (weight, bias)) adds the SEMANTIC mask at the image's own
    resolution from the tiles that were run anyway (`postprocess.seg_to_frames`): `seg_frame`, bit-packed uint8 [1, H0_n, pitch_n] per
    image (logit > `seg_threshold`), and `seg_logits`, fp32 [H0_n, W0_n].  Overlapping tiles are averaged under the `blend` window
    ("gaussian", "tent", "constant" or a float array [G]) so that no seam is left where they disagree; the full view takes part as a
    constant source.  None: not one launch changes.

    Memory: the mask coefficients and prototypes of every tile are concatenated tile-major before the vote: 32 * (S / 4)^2 fp32 = 3.3 MB
    of prototypes per tile at S = 640 (43 MB for the 13 tiles of a 2048 x 1536 image), plus 32 * A fp32 of coefficients."""
    if masks not in (False, "vote"):
        raise ValueError(f"detect_sliced: masks is False or 'vote', not {masks!r}")
    if crop and not masks:
        raise ValueError("detect_sliced: crop comes with masks='vote'")
    S = int(img_size)
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in raw_images]
    tiles = slice_geometry(sizes, S, zoom=zoom, overlap=overlap, full_view=full_view)
    x = slice_batch(raw_images, tiles, S)
    dets, mcs, protos = [], [], []
    for c0 in range(0, x.shape[0], int(batch)):
        out = model(x[c0:c0 + int(batch)], "infer")
        if "detect_features" not in out:
            raise NotImplementedError("detect_sliced drives models with a Detect head")
        _, mc, pr = out["segment_protos"]
        dets.append(detect_and_segment(out["detect_features"], mc, pr, S, conf_th, iou_th, tile_top_k, masks=False))
        if masks:
            mcs.append(mc.float())
        if masks or semantic is not None:
            protos.append(pr.float())
    det = {k: torch.cat([d[k] for d in dets]) for k in ("boxes", "scores", "labels", "counts", "keep_anchor")}
    frames = [(H0, W0, S / max(H0, W0)) for H0, W0 in sizes]
    merged = merge_tiles(det, tiles, frames, metric=metric, thr=thr, skip_thr=skip_thr, top_k=top_k, class_agnostic=class_agnostic)
    if masks:
        r = vote_tile_masks(merged, det, torch.cat(mcs), torch.cat(protos), tiles, frames, crop=crop)
        merged["masks_frame"], merged["vote_coeff"] = r["masks"], r["vote_coeff"]
        merged["_keep"] = (merged["_keep"], r["_keep"])
    if semantic is not None:
        r = seg_to_frames(torch.cat(protos), semantic, frames, tiles=tiles, blend=blend, threshold=seg_threshold, logits=True,
                          up=S / protos[0].shape[3])
        merged["seg_frame"], merged["seg_logits"], merged["_seg"] = r["masks"], r["logits"], r
    return merged
