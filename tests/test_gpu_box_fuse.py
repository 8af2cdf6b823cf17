"""`mtbt_fuse_detections` (csrc/box_fuse.hip) through `postprocess.fuse_detections` against the numpy restatement
(tests/fuse_reference.py), bit for bit on every output, the padding included."""
import numpy as np
import pytest
import torch

from fuse_reference import clustered_lists, fuse_detections as ref_fuse, orient_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import postprocess as pp

OUTPUTS = ("boxes", "scores", "labels", "counts", "n_clusters", "n_members", "lead_source", "lead_slot", "lead_anchor")


def to_dev(dets, anchors=True):
    return [{k: torch.from_numpy(v).to(DEV) for k, v in d.items() if anchors or k != "keep_anchor"} for d in dets]


def check(dets, S=640.0, anchors=True, **kw):
    """The kernel equals the restatement on every output; returns the restatement's result."""
    if not anchors:
        dets = [{k: v for k, v in d.items() if k != "keep_anchor"} for d in dets]
    want = ref_fuse(dets, S, **kw)
    got = pp.fuse_detections(to_dev(dets), img_size=S, **kw)
    torch.cuda.synchronize()
    assert sorted(k for k in got if not k.startswith("_")) == sorted(want)
    for k in want:
        g, w = got[k].cpu(), torch.from_numpy(np.asarray(want[k]))
        assert g.dtype == w.dtype and torch.equal(g, w), (k, (g != w).nonzero()[:5].tolist())
    return want


def test_main_clusters_with_several_members_and_more_members_than_sources():
    """60 objects and a +-5 px jittered copy: most clusters have one member per source at the default IoU; at IoU 0.3 the overlapping boxes of
    one source share clusters, so some hold more members than there are sources and min(n, M) decides the score."""
    dets = clustered_lists(2, 2, 100, [[60, 60], [60, 60]], seed=11)
    want = check(dets)
    for n in range(2):
        ncl = int(want["n_clusters"][n])
        assert (want["n_members"][n, :ncl] >= 2).sum() * 4 >= ncl
    low = check(dets, iou_thr=0.3)
    assert (low["n_members"] > 2).any() and (low["n_members"] >= 2).sum() * 4 >= low["n_clusters"].sum()


def test_one_box():
    d = clustered_lists(1, 1, 1, [[1]], seed=1)
    want = check(d)
    assert want["counts"][0] == 1 and np.array_equal(want["boxes"], d[0]["boxes"])


def test_identity():
    d = clustered_lists(1, 2, 100, [[60, 60]], seed=2)
    want = check(d, iou_thr=1.0)
    for k in ("boxes", "scores", "labels", "counts"):
        assert np.array_equal(want[k], d[0][k]), k
    assert np.array_equal(want["lead_anchor"], d[0]["keep_anchor"])


@pytest.mark.parametrize("orient", range(8))
def test_twins(orient):
    S, cnt = 640.0, 60
    a = clustered_lists(1, 1, 100, [[cnt]], seed=20 + orient)[0]
    b = {k: v.copy() for k, v in a.items()}
    b["boxes"] = orient_boxes(a["boxes"], orient, S)
    b["boxes"][:, cnt:] = 0
    want = check([a, b], S, orients=[0, orient], iou_thr=0.999)
    assert (want["n_members"][0, :cnt] == 2).all() and np.array_equal(want["scores"], a["scores"])
    assert np.abs(want["boxes"] - a["boxes"]).max() <= 2 * np.spacing(np.float32(S))


@pytest.mark.parametrize("K", [64, 65])
def test_wave_boundary_of_the_cluster_scan(K):
    """Three full sources of 64 / 65 slots: the cluster count passes 64, where a lane's scan takes its second cluster."""
    want = check(clustered_lists(3, 1, K, [[K]] * 3, seed=30 + K, n_centres=40, orients=[0, 3, 5]), orients=[0, 3, 5], iou_thr=0.7)
    assert want["n_clusters"][0] > 64 and (want["n_members"] >= 2).any()


def test_cap_of_4096_candidates():
    """8 full sources of 512 slots: the 4096-candidate limit, hundreds of clusters per lane scan, running sums in the workspace."""
    want = check(clustered_lists(8, 1, 512, [[512]] * 8, seed=40, n_centres=60), top_k=300)
    assert want["n_clusters"][0] > 300 and want["counts"][0] == 300 and (want["n_members"] > 8).any()


def test_2048_candidates_running_sums_in_lds():
    want = check(clustered_lists(4, 1, 512, [[512]] * 4, seed=41, n_centres=60))
    assert want["n_clusters"][0] > 128


def test_ragged_counts_and_an_empty_image():
    counts = [[60, 0, 17], [33, 0, 100], [0, 0, 64]]
    want = check(clustered_lists(3, 3, 100, counts, seed=50, orients=[0, 6, 1]), orients=[0, 6, 1], weights=[0.5, 1.0, 2.0])
    assert want["counts"][1] == 0 and want["n_clusters"][1] == 0 and want["counts"][0] > 0 and want["counts"][2] > 0


@pytest.mark.parametrize("skip_thr,some", [(0.5, True), (1.0, False)])
def test_skip_threshold(skip_thr, some):
    want = check(clustered_lists(2, 2, 100, [[60, 60], [60, 60]], seed=60), skip_thr=skip_thr)
    assert (want["counts"] > 0).all() == some and (want["n_clusters"] < 60).all()


def test_tied_scores():
    """Scores quantised to 4 values: the order is decided by the candidate index, then by the cluster index."""
    check(clustered_lists(2, 2, 100, [[100, 80], [90, 100]], seed=70, score_levels=4))
    check(clustered_lists(1, 1, 100, [[100]], seed=71, score_levels=4), iou_thr=1.0)


@pytest.mark.parametrize("nc", [1, 5])
def test_labels_never_mix(nc):
    dets = clustered_lists(2, 2, 100, [[100, 100], [100, 100]], seed=80 + nc, nc=nc)
    want = check(dets, iou_thr=0.3)
    for n in range(2):
        for r in range(int(want["counts"][n])):
            assert want["labels"][n, r] == dets[want["lead_source"][n, r]]["labels"][n, want["lead_slot"][n, r]]
    assert set(np.unique(want["labels"])) <= set(range(nc)) | {-1}


def test_weights_and_top_k_below_the_cluster_count():
    dets = clustered_lists(3, 2, 100, [[60, 60]] * 3, seed=90)
    want = check(dets, weights=[0.5, 1.0, 2.0], top_k=20)
    assert (want["n_clusters"] > 20).all() and (want["counts"] == 20).all()
    check(dets, weights=[0.5, 1.0, 2.0], top_k=300)                        # top_k above M K: padding beyond every cluster


def test_without_anchors_there_is_no_lead_anchor():
    want = check(clustered_lists(2, 1, 100, [[60], [60]], seed=95), anchors=False)
    assert "lead_anchor" not in want


def test_argument_errors():
    d = to_dev(clustered_lists(2, 2, 10, [[10, 10], [10, 10]], seed=1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        pp.fuse_detections([{k: v.cpu() for k, v in d[0].items()}], img_size=640)
    short = {k: v[:1] for k, v in d[1].items()}
    with pytest.raises(ValueError):
        pp.fuse_detections([d[0], short], img_size=640)                    # mismatched B
    narrow = {k: (v[:, :5] if v.dim() > 1 else v) for k, v in d[1].items()}
    with pytest.raises(ValueError):
        pp.fuse_detections([d[0], narrow], img_size=640)                   # mismatched K
    with pytest.raises(ValueError):
        pp.fuse_detections(d, img_size=640, weights=[1.0])
    with pytest.raises(RuntimeError, match="MTBT_EINVAL"):
        pp.fuse_detections(d, img_size=640, weights=[1.0, 0.0])
