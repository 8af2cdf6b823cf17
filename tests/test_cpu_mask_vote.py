"""CPU checks of the mask vote over fused detections: the invariants of its restatement (tests/vote_reference.py), the cases in which the
vote must agree with the single-source frame operator (tests/frame_reference.py), and the C boundary of `mtbt_vote_masks` /
`mtbt_fuse_detections_members` (struct layout, argument checks before any launch).

Bits are compared outside the band |logit| < 1e-4 * M of the case with M sources: the single-source band of the frame tests, grown
linearly with the 32 M-term sum."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import frame_reference as FR
import fuse_reference as FU
import vote_reference as VR
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, G, K, N, A = 160.0, 40, 21, 3, 300
COUNTS = [21, 3, 0]
BAND = 1e-4
FRAMES = [(97, 211, 160 / 211), (211, 97, 160 / 211), (160, 160, 1.0)]
EINVAL, EALIGN = -1, -2


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _case(M, orients, seed=3, top_k=K, skip_thr=0.0, weights=None):
    dets = FU.clustered_lists(M, N, K, [COUNTS] * M, seed, S=S, orients=orients)
    mcs, protos = VR.vote_inputs(dets, N, G, seed, orients, S=S, A=A)
    fused = VR.fuse_members(dets, S, orients, weights, skip_thr=skip_thr, top_k=top_k)
    return dets, mcs, protos, fused


def test_membership_invariants():
    for M, top_k, skip in ((1, 21, 0.0), (3, 21, 0.3), (3, 16, 0.0), (8, 16, 0.0)):
        orients = [(3 * m + 1) % 8 for m in range(M)]
        dets, _, _, fused = _case(M, orients, top_k=top_k, skip_thr=skip)
        ms = fused["member_slot"]
        assert ms.shape == (N, M * K) and ms.dtype == np.int32
        seen_cut = False
        for n in range(N):
            cnt = int(fused["counts"][n])
            assert ms[n].max(initial=-1) < cnt
            for r in range(top_k):
                assert int((ms[n] == r).sum()) == int(fused["n_members"][n, r]), (M, n, r)                # every member, once
            for r in range(cnt):
                assert ms[n, fused["lead_source"][n, r] * K + fused["lead_slot"][n, r]] == r              # the leader is a member
            live = np.concatenate([np.arange(K) < d["counts"][n] for d in dets])
            s = np.concatenate([d["scores"][n] for d in dets])
            cand = live & (s > np.float32(skip))
            assert (ms[n][~cand] == -1).all()
            cut = int(fused["n_clusters"][n]) > cnt
            seen_cut |= cut
            assert ((ms[n][cand] == -1).any()) == cut                                                    # only members of cut clusters
        assert seen_cut == (top_k == 16)
    assert (fused["n_members"] >= 2).any()


def test_single_source_is_the_frame_operator():
    dets, mcs, protos, fused = _case(1, [0])
    W, Ss = VR.vote_coefficients(dets, mcs, fused["member_slot"], fused["counts"], [1.0], K)
    vote = VR.vote_reference(W, fused["counts"], fused["boxes"], protos, [0], FRAMES, 4.0, crop=True)
    # the same rows through the frame operator: each fused row's coefficient is the score-weighted mean of its members', so compare
    # on the rows with one member (the mean of one is the member up to one rounding of s * c / s)
    d = dets[0]
    anchor = np.zeros((N, K), np.int64)
    for n in range(N):
        for r in range(int(fused["counts"][n])):
            anchor[n, r] = d["keep_anchor"][n, fused["lead_slot"][n, r]]
    ref = FR.frame_reference(protos[0], mcs[0], torch.from_numpy(anchor), fused["counts"], torch.from_numpy(fused["boxes"]), FRAMES, 4.0, crop=True)
    single = fused["n_members"] == 1
    assert single.any()
    for n in range(N):
        assert torch.equal(vote[n]["boxes"], ref[n]["boxes"])
        rows = torch.from_numpy(single[n])
        diff = (vote[n]["bits"] != ref[n]["bits"])[rows]
        assert not (diff & ~(ref[n]["logits"][rows].abs() < BAND)).any()
        assert not vote[n]["bits"][int(fused["counts"][n]):].any()


@pytest.mark.parametrize("orient", range(8))
def test_a_turned_copy_votes_like_the_source_alone(orient):
    dets, mcs, protos, fused1 = _case(1, [0])
    W1, _ = VR.vote_coefficients(dets, mcs, fused1["member_slot"], fused1["counts"], [1.0], K)
    one = VR.vote_reference(W1, fused1["counts"], fused1["boxes"], protos, [0], FRAMES[:1] * N, 4.0)
    # the second source: the same detections and coefficients seen through `orient` (boxes and prototypes turned)
    turned = dict(dets[0])
    turned["boxes"] = FU.orient_boxes(dets[0]["boxes"], orient, S)
    turned["boxes"][np.arange(K)[None, :] >= dets[0]["counts"][:, None]] = 0
    both, orients = [dets[0], turned], [0, orient]
    fused2 = VR.fuse_members(both, S, orients, None, top_k=K)
    # every cluster gets each member twice; its box is the same up to the rounding of (s b + s b) / (s + s)
    assert np.allclose(fused2["boxes"], fused1["boxes"], rtol=1e-6, atol=0) and np.array_equal(fused2["n_members"], 2 * fused1["n_members"])
    W2, _ = VR.vote_coefficients(both, [mcs[0], mcs[0]], fused2["member_slot"], fused2["counts"], [1.0, 1.0], K)
    two = VR.vote_reference(W2, fused2["counts"], fused2["boxes"], [protos[0], VR.orient_protos(protos[0], orient)], orients, FRAMES[:1] * N, 4.0)
    for n in range(N):
        diff = one[n]["bits"] != two[n]["bits"]
        assert not (diff & ~(one[n]["logits"].abs() < 2 * BAND)).any()
        assert one[n]["bits"].any() or int(fused1["counts"][n]) == 0


def test_struct_layout_matches_header(lib, tmp_path):
    assert lib.mtbt_sizeof_vote_mask_args() == C.sizeof(L.VoteMaskArgs)
    fields = ["protos", "mc", "mc_batch_stride", "mc_k_stride", "mc_c_stride", "anchors", "scores", "weight", "orient", "member_slot", "counts",
              "boxes", "boxes_frame", "W", "Ss", "out", "out_bytes", "n_sources", "N", "K", "top_k", "nm", "hp", "wp", "crop"]
    assert fields == [f[0] for f in L.VoteMaskArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(mtbt_vote_mask_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbt_vote_mask_args, {f}));' for f in fields]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.VoteMaskArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.VoteMaskArgs, f).offset, f


def _vote_args(M=2):
    """Arguments that pass every check of mtbt_vote_masks (dummy non-null, 16-byte aligned pointers: nothing may be launched)."""
    a = L.VoteMaskArgs()
    for m in range(M):
        a.protos[m] = a.mc[m] = a.anchors[m] = a.scores[m] = 16
        a.mc_batch_stride[m], a.mc_k_stride[m], a.mc_c_stride[m] = 32 * A, 1, A
        a.weight[m], a.orient[m] = 1.0, m
    a.member_slot = a.counts = a.boxes = a.boxes_frame = a.W = a.Ss = a.out = 16
    a.n_sources, a.N, a.K, a.top_k, a.nm, a.hp, a.wp, a.crop = M, 1, K, K, 32, G, G, 1
    fr = (L.Frame * 1)()
    fr[0].height, fr[0].width, fr[0].step, fr[0].scale, fr[0].pitch, fr[0].offset = 160, 160, 0.25, 1.0, 24, 0
    a.out_bytes = K * 160 * 24
    return a, fr


def test_vote_masks_rejects_bad_arguments_without_launching(lib):
    def run(edit, fr_edit=None, n_frames=1):
        a, fr = _vote_args()
        edit(a)
        if fr_edit:
            fr_edit(fr[0])
        return lib.mtbt_vote_masks(C.byref(a), fr, n_frames, None)

    assert lib.mtbt_vote_masks(None, None, 1, None) == EINVAL
    a, fr = _vote_args()
    assert lib.mtbt_vote_masks(C.byref(a), None, 1, None) == EINVAL
    # every EINVAL is reported although protos[0] is misaligned too: the alignment check comes last
    def bad(**kw):
        def edit(a):
            a.protos[0] = 24
            for k, v in kw.items():
                setattr(a, k, v)
        return edit
    for kw in (dict(hp=G + 1), dict(wp=G - 1), dict(hp=0, wp=0), dict(n_sources=0), dict(n_sources=9), dict(nm=16), dict(K=0), dict(K=4096),
               dict(top_k=0), dict(top_k=65536), dict(N=2), dict(out_bytes=-1), dict(out_bytes=K * 160 * 24 - 1), dict(member_slot=None),
               dict(counts=None), dict(W=None), dict(Ss=None), dict(out=None), dict(boxes=None)):
        assert run(bad(**kw)) == EINVAL, kw
    for name in ("protos", "mc", "anchors", "scores"):
        for m in (0, 1):
            def edit(a, name=name, m=m):
                a.protos[0] = 24
                getattr(a, name)[m] = None
            assert run(edit) == EINVAL, (name, m)
    for o in (-1, 8):
        def edit(a, o=o):
            a.protos[0] = 24
            a.orient[1] = o
        assert run(edit) == EINVAL, o
    for fe in (lambda f: setattr(f, "step", 1.5), lambda f: setattr(f, "step", 0.0), lambda f: setattr(f, "pitch", 16),
               lambda f: setattr(f, "offset", 8), lambda f: setattr(f, "scale", 0.0), lambda f: setattr(f, "height", 0)):
        assert run(bad(), fe) == EINVAL
    assert run(lambda a: None, n_frames=0) == EINVAL and run(lambda a: None, n_frames=33) == EINVAL
    # then the alignment
    assert run(bad()) == EALIGN
    def edit(a):
        a.protos[1] = 24
    assert run(edit) == EALIGN
    assert run(lambda a: setattr(a, "out", 24)) == EALIGN


def test_fuse_members_rejects_bad_arguments_without_launching(lib):
    a = L.BoxFuseArgs()
    for m in range(2):
        a.boxes[m] = a.scores[m] = a.labels[m] = a.counts[m] = a.anchors[m] = 16
        a.orient[m], a.weight[m] = m, 1.0
    a.n_sources, a.N, a.K, a.top_k, a.img_size, a.iou_thr = 2, 1, K, K, 160.0, 0.55
    a.out_boxes = a.out_scores = a.out_labels = a.out_counts = a.n_clusters = a.n_members = a.lead_source = a.lead_slot = a.workspace = 16
    a.workspace_bytes = lib.mtbt_fuse_workspace_bytes(2, 1, K)
    assert lib.mtbt_fuse_detections_members(None, 16, None) == EINVAL
    a.boxes[1] = 24                                    # misaligned: reported only once everything else is in order
    assert lib.mtbt_fuse_detections_members(C.byref(a), None, None) == EINVAL      # NULL member_slot
    assert lib.mtbt_fuse_detections_members(C.byref(a), 16, None) == EALIGN
    assert lib.mtbt_fuse_detections(C.byref(a), None) == EALIGN                    # the member-less entry never looks at it
    a.orient[1] = 8
    assert lib.mtbt_fuse_detections_members(C.byref(a), 16, None) == EINVAL
    a.orient[1], a.N = 1, 0
    assert lib.mtbt_fuse_detections_members(C.byref(a), None, None) == 0           # N == 0 returns before the pointers are looked at
