"""The task-aligned detection loss without a GPU: the CPU restatement (tests/tal_reference.py) against an independent per-GT,
per-anchor loop, the properties of the assignment, the margin condition that makes an exact comparison of assignments on the GPU
legitimate, and the C ABI of the operator (struct layout against the compiled header, argument checks before any launch)."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import mask_loss_reference as M
import tal_reference as R

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK, ALPHA, BETA = 10, 0.5, 6.0
CASES = [1, 2, 3, 4, 5]


def _ciou(p, g, eps=1e-7):
    wp, hp = p[2] - p[0], p[3] - p[1] + eps
    wg, hg = g[2] - g[0], g[3] - g[1] + eps
    inter = max(min(p[2], g[2]) - max(p[0], g[0]), 0.0) * max(min(p[3], g[3]) - max(p[1], g[1]), 0.0)
    iou = inter / (wp * hp + wg * hg - inter + eps)
    cw, ch = max(p[2], g[2]) - min(p[0], g[0]), max(p[3], g[3]) - min(p[1], g[1])
    rho2 = ((g[0] + g[2] - p[0] - p[2]) ** 2 + (g[1] + g[3] - p[1] - p[3]) ** 2) / 4
    v = 4 / math.pi ** 2 * (math.atan(wg / hg) - math.atan(wp / hp)) ** 2
    return iou - (rho2 / (cw * cw + ch * ch + eps) + v * (v / (v - iou + 1 + eps)))


def _bce(x, t):
    return max(x, 0.0) - x * t + math.log1p(math.exp(-abs(x)))


def loop_loss(c):
    """The definition as plain Python loops in double precision over the decoded boxes: (box, dfl, cls, n_fg, mean ov, assigned)."""
    S, reg_max = c["kw"]["img_size"], c["kw"]["reg_max"]
    det = c["det"]
    boxes = M.decode_boxes(det, S, reg_max).double().tolist()
    raw, cls = R.rows_of(det, reg_max)
    raw, cls = raw.double(), cls.double().tolist()
    pts, st = R.anchors_of(det, S)
    pts, st = pts.double().tolist(), st.double().tolist()
    Bn, A = len(boxes), len(pts)
    assigned = [[-1] * A for _ in range(Bn)]
    tsc = [[0.0] * A for _ in range(Bn)]
    ovs = [[0.0] * A for _ in range(Bn)]
    gts, off = [], 0
    for b in range(Bn):
        gx, gc = R.gt_of(c["gt"], b, S)
        gx, gc = gx.double().tolist(), gc.tolist()
        chosen = {}                                           # anchor -> [(g, ov, metric)]
        per_g = []
        for g, (bx, k) in enumerate(zip(gx, gc)):
            rows = []
            for a in range(A):
                ax, ay = pts[a]
                inside = min(ax - bx[0], ay - bx[1], bx[2] - ax, bx[3] - ay) > 1e-9
                ov = max(_ciou(boxes[b][a], bx), 0.0) if inside else 0.0
                metric = (1 / (1 + math.exp(-cls[b][a][k]))) ** ALPHA * ov ** BETA
                rows.append((metric, ov, inside))
            order = sorted(range(A), key=lambda a: (-rows[a][0], a))[:TOPK]
            for a in order:
                if rows[a][2]:
                    chosen.setdefault(a, []).append((g, rows[a][1], rows[a][0]))
            per_g.append(rows)
        fg_of = {}
        for a, cands in chosen.items():
            g = max(cands, key=lambda t: (t[1], -t[0]))[0]
            assigned[b][a] = g + off
            fg_of.setdefault(g, []).append(a)
        for g, al in fg_of.items():
            Mg, Og = max(per_g[g][a][0] for a in al), max(per_g[g][a][1] for a in al)
            for a in al:
                tsc[b][a] = per_g[g][a][0] * Og / (Mg + 1e-9)
                ovs[b][a] = per_g[g][a][1]
        gts.append((gx, gc, off))
        off += len(gx)
    T = max(sum(sum(r) for r in tsc), 1.0)
    box = dfl = cl = ov_sum = 0.0
    n_fg = 0
    for b in range(Bn):
        gx, gc, off = gts[b]
        for a in range(A):
            g = assigned[b][a]
            t = tsc[b][a]
            k = gc[g - off] if g >= 0 else -1
            cl += sum(_bce(x, t if j == k else 0.0) for j, x in enumerate(cls[b][a]))
            if g < 0:
                continue
            bx = gx[g - off]
            n_fg += 1
            ov_sum += ovs[b][a]
            box += (1 - _ciou(boxes[b][a], bx)) * t
            ax, ay = pts[a]
            side = 0.0
            for s, dist in enumerate((ax - bx[0], ay - bx[1], bx[2] - ax, bx[3] - ay)):
                tg = min(max(dist / st[a], 0.0), reg_max - 1 - 0.01)
                tl = int(math.floor(tg))
                wl = tl + 1 - tg
                lp = torch.log_softmax(raw[b, a, s], 0).tolist()
                side += -(lp[tl] * wl + lp[tl + 1] * (1 - wl))
            dfl += t * side / 4
    return box / T, dfl / T, cl / T, n_fg, (ov_sum / n_fg if n_fg else 0.0), assigned


@pytest.mark.parametrize("k", CASES)
def test_restatement_equals_an_independent_loop(k):
    ref = R.reference(k)
    box, dfl, cl, n_fg, mov, assigned = loop_loss(R.case(k))
    assert ref["asg"]["assigned"].tolist() == assigned
    assert ref["values"][3] == n_fg
    for name, got, want in zip(("box", "dfl", "cls", "mean ov"), (ref["values"][0], ref["values"][1], ref["values"][2], ref["values"][4]),
                               (box, dfl, cl, mov)):
        print(f"case {k} {name}: restatement {got:.7f} loop {want:.7f}")
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (name, got, want)
    if k in (1, 2, 3, 5):
        assert n_fg > 0
    else:
        assert n_fg == 0 and ref["values"][0] == 0.0 and ref["values"][1] == 0.0 and ref["values"][4] == 0.0 and ref["values"][2] > 0


@pytest.mark.parametrize("k", CASES)
def test_assignment_properties(k):
    ref = R.reference(k)
    asg = ref["asg"]
    B_ = asg["assigned"].shape[0]
    for b in range(B_):
        per = asg["per"][b]
        a_b = asg["assigned"][b]
        if per is None:
            assert (a_b < 0).all() and not asg["t"][b].any()
            continue
        g = per["metric"].shape[0]
        for r in range(g):
            mine = torch.nonzero(a_b == r + asg["off"][b]).flatten()
            assert per["inside"][r][mine].all()                       # every fg anchor is inside its GT
            assert mine.numel() <= TOPK
            if mine.numel():
                # the largest target score of a GT is its largest overlap, up to the 1e-9 of the definition's denominator (which
                # matters for a GT whose best metric is itself tiny: overlap^6)
                Og, Mg = per["Og"][r].item(), per["Mg"][r].item()
                assert abs(asg["t"][b][mine].max().item() - Og * Mg / (Mg + 1e-9)) <= 1e-6 * max(Og, 1e-30)
    # background anchors are pushed down: their class gradient is not zero, their distribution gradient is
    bg = asg["assigned"] < 0
    flat = torch.cat([d.permute(0, 2, 3, 1).reshape(d.shape[0], -1, d.shape[1]) for d in ref["grads"]], 1)
    assert bg.any() and (flat[bg][:, 64:] != 0).all()
    assert not flat[bg][:, :64].any()


def test_case_5_has_a_gt_without_anchors_and_a_skipped_row():
    asg = R.reference(5)["asg"]
    gx, _ = asg["rows"][1]
    assert gx.shape[0] == 1                                           # the zero-width row is skipped
    assert not asg["per"][1]["inside"].any() and (asg["assigned"][1] < 0).all()
    assert torch.equal(asg["assigned"][0], R.reference(1)["asg"]["assigned"][0])


def test_the_cases_cover_the_paths():
    """Images without GT, a GT with fewer inside anchors than topk, GTs with hundreds of candidates, contested anchors resolved in
    both directions."""
    few = many = empty = 0
    directions = set()
    for k in (1, 2, 3):
        asg = R.reference(k)["asg"]
        empty += sum(p is None for p in asg["per"])
        for per in asg["per"]:
            if per is None:
                continue
            n_in = per["inside"].sum(1)
            few += int(((n_in > 0) & (n_in < TOPK)).sum())
            many += int((n_in >= 200).sum())
            contested = torch.nonzero(per["sel"].sum(0) > 1).flatten()
            for a in contested.tolist():
                directions.add(int(torch.nonzero(per["final"][:, a]).item()))
    assert empty >= 1 and few >= 1 and many >= 1 and len(directions) >= 2


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_margin_condition(k):
    """What lets the GPU test compare assignments exactly: the 10th and 11th metric of every GT with more than topk positive metrics
    differ by >= 1e-4 (relative), and the two largest overlaps at every contested anchor by >= 1e-4."""
    asg = R.reference(k)["asg"]
    tight_m = tight_o = float("inf")
    for per in asg["per"]:
        if per is None:
            continue
        srt = torch.sort(per["metric"], dim=1, descending=True, stable=True).values
        for r in range(srt.shape[0]):
            if srt.shape[1] > TOPK and srt[r, TOPK] > 0:
                tight_m = min(tight_m, ((srt[r, TOPK - 1] - srt[r, TOPK]) / srt[r, TOPK - 1]).item())
        for a in torch.nonzero(per["sel"].sum(0) > 1).flatten().tolist():
            o = torch.sort(per["ov"][per["sel"][:, a], a], descending=True).values
            tight_o = min(tight_o, (o[0] - o[1]).item())
    print(f"case {k}: tightest relative metric gap {tight_m:.3e}, tightest contested overlap gap {tight_o:.3e}")
    assert tight_m >= 1e-4 and tight_o >= 1e-4


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def test_struct_layout_matches_the_header(tmp_path, lib):
    fields = [f for f, _ in L.TalLossArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){',
             'printf("sizeof %zu\\n", sizeof(mtbt_tal_loss_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbt_tal_loss_args, {f}));' for f in fields]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.TalLossArgs) == lib.mtbt_sizeof_tal_loss_args()
    for f in fields:
        assert int(out[f]) == getattr(L.TalLossArgs, f).offset, f


def test_entry_points_reject_bad_arguments_without_launching(lib):
    assert lib.mtbt_tal_det_loss(None, None) == -1
    assert lib.mtbt_tal_det_loss(C.byref(L.TalLossArgs()), None) == -1
    assert lib.mtbt_tal_loss_workspace_bytes(0, 84, 3) == 0 and lib.mtbt_tal_loss_workspace_bytes(2, 0, 3) == 0
    assert lib.mtbt_tal_loss_workspace_bytes(2, 84, -1) == 0
    assert lib.mtbt_tal_loss_workspace_bytes(2, 8400, 5) >= 2 * 8400 * (16 + 64 + 8) + 5 * 8400 * 8
    a = L.TalLossArgs()
    a.gt_xyxy = a.gt_cls = a.gt_off = a.out = a.workspace = 16           # non-null dummies: the size checks must fire first
    a.map[0], a.h[0], a.w[0], a.map_pixel_stride[0] = 16, 8, 8, 66
    a.n_levels, a.N, a.nc, a.reg_max, a.img_size, a.n_gt, a.topk = 1, 1, 2, 16, 64.0, 1, 10
    a.workspace_bytes = 0
    assert lib.mtbt_tal_det_loss(C.byref(a), None) == -4                 # workspace too small
    a.workspace_bytes = lib.mtbt_tal_loss_workspace_bytes(1, 64, 1)
    for field, bad in (("topk", 0), ("topk", 65), ("n_gt", -1), ("n_levels", 4), ("N", 0), ("nc", 0), ("reg_max", 0)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.mtbt_tal_det_loss(C.byref(a), None) == -1, field
        setattr(a, field, good)
    a.map_pixel_stride[0] = 65                                           # narrower than 4 * reg_max + nc
    assert lib.mtbt_tal_det_loss(C.byref(a), None) == -1
    a.map_pixel_stride[0] = 66
    a.gt_xyxy = 20
    assert lib.mtbt_tal_det_loss(C.byref(a), None) == -2                 # misaligned
    a.gt_xyxy = 16
    a.d_map[0], a.d_map_pixel_stride[0] = 16, 65
    assert lib.mtbt_tal_det_loss(C.byref(a), None) == -1


def test_trainstep_rejects_an_unknown_det_loss():
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    with pytest.raises(ValueError, match="det_loss"):
        TrainStep(None, (2, 3, 128, 128), det_loss="hungarian")
    with pytest.raises(ValueError, match="tal"):
        TrainStep(None, (2, 3, 128, 128), tal=dict(topk=13))
