"""Weighted boxes fusion without a GPU: the numpy restatement (tests/fuse_reference.py) of `mtbt_fuse_detections` on the identities the
definition guarantees bit for bit, a hand-worked case with literal values, the NaN overlap of zero-area boxes, and the argument checks of
the library, which refuse a bad call before any launch.  The arithmetic is the project's own definition (include/mtbt_hip.h)."""
import ctypes as C

import numpy as np
import pytest

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

from fuse_reference import clustered_lists, fuse_detections, fuse_image, orient_boxes, unorient

EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch
F = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_identity_every_candidate_is_its_own_cluster():
    """M = 1, weight 1, orient 0, iou_thr = 1.0: `> 1.0` never holds (identical boxes included), the output is the input in score
    order with score == s."""
    K, cnt = 100, 60
    d = clustered_lists(1, 2, K, [[cnt, cnt]], seed=1)[0]
    d["boxes"][0, 7] = d["boxes"][0, 3]           # identical boxes, same label: ovr == 1.0 exactly, still not > 1.0
    d["labels"][0, 7] = d["labels"][0, 3]
    out = fuse_detections([d], 640.0, iou_thr=1.0)
    for k in ("boxes", "scores", "labels", "counts"):
        assert np.array_equal(out[k], d[k]), k
    assert np.array_equal(out["lead_anchor"], d["keep_anchor"])
    assert (out["n_clusters"] == cnt).all() and (out["n_members"][:, :cnt] == 1).all() and (out["n_members"][:, cnt:] == 0).all()
    assert (out["lead_source"][:, :cnt] == 0).all() and (out["lead_slot"][:, :cnt] == np.arange(cnt)).all()
    assert (out["lead_source"][:, cnt:] == -1).all() and (out["lead_slot"][:, cnt:] == -1).all()


@pytest.mark.parametrize("orient", range(8))
def test_twins_fuse_to_the_input_score(orient):
    """Two sources hold the same list, the second in the frame of view `orient`: with iou_thr = 0.999 every cluster has exactly 2 members,
    the fused score equals the input score exactly and the coordinates agree within 2 ulp of img_size."""
    S, K, cnt = 640.0, 100, 60
    a = clustered_lists(1, 1, K, [[cnt]], seed=2 + orient)[0]
    b = {k: v.copy() for k, v in a.items()}
    b["boxes"] = orient_boxes(a["boxes"], orient, S)
    b["boxes"][:, cnt:] = 0
    assert np.array_equal(unorient(b["boxes"][0, :cnt], orient, S), a["boxes"][0, :cnt])        # 1/8 px coordinates: S - x is exact
    out = fuse_detections([a, b], S, orients=[0, orient], iou_thr=0.999)
    assert out["n_clusters"][0] == cnt and (out["n_members"][0, :cnt] == 2).all()
    assert np.array_equal(out["scores"], a["scores"]) and np.array_equal(out["labels"], a["labels"])
    assert (out["lead_source"][0, :cnt] == 0).all() and np.array_equal(out["lead_slot"][0, :cnt], np.arange(cnt))
    assert np.abs(out["boxes"] - a["boxes"]).max() <= 2 * np.spacing(F(S))                       # round(s x) / s: two roundings


def test_hand_worked_five_boxes():
    """Scores are binary fractions that sum to 1 in the big cluster, so every figure below is exact.  Order by (score desc, c asc):
    a (c 0, .5), b (c 1, .25), d (c 3, .25), c (c 2, .125), e (c 4, .0625).  a opens cluster 0; b joins it (IoU 360 / 440); d joins the
    fused (10.67, 10, 30.67, 30) box (IoU 348 / 452): three members from two sources, so min(n, M) = 2 matters; c has another label and
    opens cluster 1; e lies exactly on c but carries label 0, overlaps cluster 0 by nothing and opens cluster 2."""
    K = 3
    src0 = (np.array([[10, 10, 30, 30], [12, 10, 32, 30], [60, 60, 80, 80]], F), np.array([0.5, 0.25, 0.125], F), np.array([0, 0, 1]), 3,
            np.array([11, 22, 33], np.int32))
    src1 = (np.array([[10, 12, 30, 32], [60, 60, 80, 80], [0, 0, 0, 0]], F), np.array([0.25, 0.0625, 0], F), np.array([0, 0, -1]), 2,
            np.array([44, 55, -1], np.int32))
    out = fuse_image([src0, src1], [0, 0], [1.0, 1.0], 100.0, 0.5, 0.0, 4, K)
    assert out["counts"] == 3 and out["n_clusters"] == 3
    assert np.array_equal(out["boxes"], np.array([[10.5, 10.5, 30.5, 30.5], [60, 60, 80, 80], [60, 60, 80, 80], [0, 0, 0, 0]], F))
    assert np.array_equal(out["scores"], np.array([0.33333334, 0.0625, 0.03125, 0], F))     # ((1 / 3) * 2) / 2, (.125 / 1 * 1) / 2, ...
    assert out["labels"].tolist() == [0, 1, 0, -1]
    assert out["n_members"].tolist() == [3, 1, 1, 0]
    assert out["lead_source"].tolist() == [0, 0, 1, -1] and out["lead_slot"].tolist() == [0, 2, 1, -1]
    assert out["lead_anchor"].tolist() == [11, 33, 55, -1]
    # without the count correction the three-member cluster would score (1 / 3 * 3) / 2 = 0.5
    assert out["scores"][0] != F(0.5)
    # top_k below the cluster count cuts the output, not the clustering
    cut = fuse_image([src0, src1], [0, 0], [1.0, 1.0], 100.0, 0.5, 0.0, 2, K)
    assert cut["counts"] == 2 and cut["n_clusters"] == 3 and np.array_equal(cut["scores"], out["scores"][:2])
    # weights scale the scores before the threshold: source 1 at weight 2 -> d (.5) ties with a and sorts after it (c 3 > c 0)
    w = fuse_image([src0, src1], [0, 0], [1.0, 2.0], 100.0, 0.5, 0.1, 4, K)
    assert w["n_clusters"] == 3 and w["lead_source"].tolist()[:3] == [0, 0, 1]               # e: .0625 * 2 = .125 > .1 stays
    assert w["scores"][0] == ((F(1.25) / F(3)) * F(2)) / F(3)


def test_zero_area_boxes_never_join():
    """inter / union = 0 / 0 = NaN for two identical zero-area boxes: a NaN never wins, the second opens its own cluster."""
    src = (np.array([[5, 5, 5, 5], [5, 5, 5, 5]], F), np.array([0.75, 0.5], F), np.array([0, 0]), 2, None)
    out = fuse_image([src], [0], [1.0], 64.0, 0.0, 0.0, 2, 2)
    assert out["n_clusters"] == 2 and out["n_members"].tolist() == [1, 1] and "lead_anchor" not in out
    assert out["scores"].tolist() == [0.75, 0.5]


def test_skip_threshold_and_label_separation():
    d = clustered_lists(2, 1, 40, [[40], [40]], seed=9, nc=5)
    out = fuse_detections(d, 640.0, iou_thr=0.3)
    n = int(out["counts"][0])
    for r in range(n):                                           # a cluster carries its leader's label
        assert out["labels"][0, r] == d[out["lead_source"][0, r]]["labels"][0, out["lead_slot"][0, r]]
    assert (out["n_members"][0, :n] >= 2).sum() >= n // 4
    assert fuse_detections(d, 640.0, skip_thr=0.5)["n_members"].sum() == sum((x["scores"] > 0.5).sum() for x in d)
    assert fuse_detections(d, 640.0, skip_thr=1.0)["counts"][0] == 0


# ---- the library ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _args(M=2, N=2, K=100, top_k=100):
    a = L.BoxFuseArgs()
    for m in range(M):
        a.boxes[m] = a.scores[m] = a.labels[m] = a.counts[m] = a.anchors[m] = PTR
        a.orient[m], a.weight[m] = m % 8, 1.0
    a.n_sources, a.N, a.K, a.top_k = M, N, K, top_k
    a.img_size, a.iou_thr, a.skip_thr = 640.0, 0.55, 0.0
    for f in ("out_boxes", "out_scores", "out_labels", "out_counts", "n_clusters", "n_members", "lead_source", "lead_slot", "lead_anchor", "workspace"):
        setattr(a, f, PTR)
    a.workspace_bytes = 1 << 40
    return a


def test_symbols_and_workspace(lib):
    assert lib.mtbt_sizeof_box_fuse_args() == C.sizeof(L.BoxFuseArgs)
    assert lib.mtbt_fuse_workspace_bytes(2, 16, 100) >= 16 * 200 * 32
    assert lib.mtbt_fuse_workspace_bytes(8, 1, 512) >= 4096 * 32
    for bad in ((0, 1, 100), (9, 1, 100), (8, 1, 513), (2, 0, 100), (2, 1, 0)):
        assert lib.mtbt_fuse_workspace_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_before_any_launch(lib):
    assert lib.mtbt_fuse_detections(None, None) == EINVAL

    def rc(edit, **kw):
        a = _args(**kw)
        edit(a)
        return lib.mtbt_fuse_detections(C.byref(a), None)

    assert rc(lambda a: setattr(a, "n_sources", 0)) == EINVAL
    assert rc(lambda a: setattr(a, "n_sources", 9)) == EINVAL
    assert rc(lambda a: None, M=8, K=513) == EINVAL                       # M K > 4096
    assert rc(lambda a: setattr(a, "top_k", 0)) == EINVAL
    assert rc(lambda a: setattr(a, "K", 0)) == EINVAL
    assert rc(lambda a: setattr(a, "N", -1)) == EINVAL
    for o in (-1, 8):
        assert rc(lambda a: a.orient.__setitem__(1, o)) == EINVAL
    for w in (0.0, -1.0, float("nan")):
        assert rc(lambda a: a.weight.__setitem__(0, w)) == EINVAL
    for s in (0.0, -640.0, float("nan")):
        assert rc(lambda a: setattr(a, "img_size", s)) == EINVAL
    for f in ("boxes", "scores", "labels", "counts"):
        assert rc(lambda a: getattr(a, f).__setitem__(1, None)) == EINVAL, f
    for f in ("out_boxes", "out_scores", "out_labels", "out_counts", "n_clusters", "n_members", "lead_source", "lead_slot", "workspace"):
        assert rc(lambda a: setattr(a, f, None)) == EINVAL, f
    assert rc(lambda a: a.anchors.__setitem__(1, None)) == EINVAL          # lead_anchor wanted, a source without anchors
    assert rc(lambda a: setattr(a, "workspace_bytes", lib.mtbt_fuse_workspace_bytes(2, 2, 100) - 1)) == EINVAL
    assert rc(lambda a: a.boxes.__setitem__(1, PTR + 4)) == EALIGN
    assert rc(lambda a: setattr(a, "out_boxes", PTR + 8)) == EALIGN
    assert rc(lambda a: a.boxes.__setitem__(1, PTR + 4), N=0) == 0          # N = 0: a successful no-op, nothing is touched
    bad = _args(N=0)
    bad.top_k = 0
    assert lib.mtbt_fuse_detections(C.byref(bad), None) == EINVAL          # ... but the scalar checks come first
