"""The float64 restatements of the refinement report's geometry (host/evaluate.py: cuboid_iou_torch, layout_overlap_torch,
visible_rows, room_rows) against tests/golden/refine_report.npz - the reference's own get_boxes / get_iou_cuboid executed from its
source text (tools/gen_golden_refine_report.py; the Polygon stand-in is the one restated piece) - and against known answers.
CPU only.  Tolerance: the project's standing rule (tests/parity.py); the recorded IoUs come from float32 corners, the restatement
builds them in float64 from the same float32 boxes."""
import json
import math
import os
import re

import numpy as np
import torch

from conftest import ROOT, load_golden, pkg
from parity import assert_close


def _meta(g):
    return json.loads(bytes(g["meta"]).decode())


def _rooms_of_single(n):
    return torch.full((n,), n - 1, dtype=torch.int32)


def test_entry_points_are_declared():
    L = pkg("_lib")
    txt = open(os.path.join(ROOT, "include", "sln_hip.h")).read()
    for name in ("sln_layout_cuboid_iou", "sln_layout_overlap", "sln_refine_report", "sln_refine_report_scratch_doubles"):
        assert name in L.SIGNATURES and re.search(r"\b%s\s*\(" % name, txt), name
    E = pkg("host.evaluate")
    for f in ("visible_rows", "room_rows", "cuboid_iou", "layout_overlap", "cuboid_iou_torch", "layout_overlap_torch"):
        assert callable(getattr(E, f))


def test_hand_cases_match_the_executed_reference():
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    m = _meta(g)
    for name in m["hand"]:
        p = "hand:%s:" % name
        objs = torch.from_numpy(g[p + "objs"])
        kept = g[p + "kept"]
        vis = E.visible_rows(objs, m["names"])
        assert torch.nonzero(vis).flatten().tolist() == kept.tolist(), name          # the rows the executed get_boxes kept
        if not len(kept):
            continue
        n = len(objs)
        iou, mean = E.cuboid_iou_torch(torch.from_numpy(g[p + "boxes"])[None], torch.from_numpy(g[p + "angles"])[None],
                                       torch.from_numpy(g[p + "gt_boxes"]), torch.from_numpy(g[p + "gt_angles"]), _rooms_of_single(n), vis)
        print(name, iou[0, kept].tolist(), g[p + "iou"].tolist())
        assert_close(iou[0, kept].numpy(), g[p + "iou"], "hand case " + name)
        assert_close(mean[0, 0].numpy(), np.mean(g[p + "iou"]), "mean of " + name)


def test_random_pairs_match_the_executed_reference():
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    iou, mean = E.cuboid_iou_torch(torch.from_numpy(g["rand:boxes"])[None], torch.from_numpy(g["rand:angles"])[None],
                                   torch.from_numpy(g["rand:gt_boxes"]), torch.from_numpy(g["rand:gt_angles"]), torch.from_numpy(g["rand:room_of_row"]))
    err = np.abs(iou[0].numpy() - g["rand:iou"])
    print("random pairs: max err %.3e at row %d" % (err.max(), int(err.argmax())))
    assert_close(iou[0].numpy(), g["rand:iou"], "2000 random pairs")
    rr = g["rand:room_of_row"]
    want = np.asarray([g["rand:iou"][rr == r].mean() for r in np.unique(rr)])
    assert_close(mean[0].numpy(), want, "per-room means")


def test_loop_records_match():
    """the per-iteration IoU of the reference's k loop from the committed loop fixtures' boxes / idx"""
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    m = _meta(g)
    for case, n_rooms in m["loops"].items():
        lg = load_golden(case)
        for r in range(n_rooms):
            p, q = "room%d:" % r, "loop:%s:room%d:" % (case, r)
            objs = torch.from_numpy(lg[p + "objs"])
            vis = E.visible_rows(objs, m["names"])
            assert torch.nonzero(vis).flatten().tolist() == g[q + "kept"].tolist()
            iou, mean = E.cuboid_iou_torch(torch.from_numpy(lg[p + "boxes"]), torch.from_numpy(lg[p + "idx"]), torch.from_numpy(lg[p + "in_boxes"]),
                                           torch.from_numpy(lg[p + "in_angles"]).float(), _rooms_of_single(len(objs)), vis)
            assert_close(iou[:, g[q + "kept"]].numpy(), g[q + "ious"], "%s room %d rows" % (case, r))
            assert_close(mean[:, 0].numpy(), g[q + "iou"], "%s room %d means" % (case, r))


def test_known_answers():
    E = pkg("host.evaluate")
    s, h = 0.4, 0.6                                                       # a 0.2 x 0.3 x 0.2 box in a room of extent 2: 0.4 x 0.6 x 0.4
    room = [0, 0, 0, 2.0, 2.0, 2.0]
    sq = [0.2, 0.0, 0.2, 0.4, 0.3, 0.4]
    gt = torch.tensor([sq, sq, [0.1, 0.0, 0.1, 0.7, 0.6, 0.7], room])
    b = torch.tensor([[sq, sq, [0.3, 0.1, 0.3, 0.5, 0.4, 0.5], room]])
    iou, _ = E.cuboid_iou_torch(b, torch.tensor([[3.0, 0, 0, 0]]), gt, torch.zeros(4), _rooms_of_single(4))
    v = s * s * h
    octagon = 2 * (math.sqrt(2) - 1) * s * s * h
    # (the boxes are float32: 0.2f, 0.3f, 0.4f are off their decimal values by up to 6e-8 relative, a volume by 2e-7: bound 1e-6)
    assert abs(float(iou[0, 0]) - octagon / (2 * v - octagon + 1e-5)) < 1e-6
    assert abs(float(iou[0, 1]) - v / (v + 1e-5)) < 1e-6                    # identical
    big, small = 1.2 * 1.2 * 1.2, 0.4 * 0.6 * 0.4
    assert abs(float(iou[0, 2]) - small / (big + 1e-5)) < 1e-6               # containment: the volume ratio


def test_invariances():
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    b, a = torch.from_numpy(g["rand:boxes"])[None], torch.from_numpy(g["rand:angles"])[None]
    gb, ga, rr = torch.from_numpy(g["rand:gt_boxes"]), torch.from_numpy(g["rand:gt_angles"]), torch.from_numpy(g["rand:room_of_row"])
    iou, _ = E.cuboid_iou_torch(b, a, gb, ga, rr)
    swapped, _ = E.cuboid_iou_torch(gb[None], ga[None], b[0], a[0], rr)
    assert_close(swapped.numpy(), iou.numpy(), "swapping the two cuboids", rtol=0, atol=1e-9)
    # 24 * float32(2 pi / 24) misses 2 pi by up to 24 * 0.26 * 6e-8 = 4e-7 rad; a corner at distance <= 1 from its centre moves by as
    # much, and an IoU changes by a few times a corner's displacement over the box size (>= 0.1 here): bound 1e-5
    turned, _ = E.cuboid_iou_torch(b, a.double() + 24.0, gb, ga, rr)
    assert_close(turned.numpy(), iou.numpy(), "a turn by 24 bins", rtol=0, atol=1e-5)


def test_layout_overlap_is_the_double_loop():
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    rows = slice(0, 63)                                                     # three rooms of 21 rows
    b, a = torch.from_numpy(g["rand:boxes"][rows]), torch.from_numpy(g["rand:angles"][rows])
    rr = torch.from_numpy(g["rand:room_of_row"][rows])
    vis = torch.ones(63, dtype=torch.bool)
    vis[[3, 20, 30]] = False                                                # (row 20: a room row)
    thresh = 0.05
    vol, pairs, _ = E.layout_overlap_torch(b[None], a[None], rr, vis, thresh)
    want_v, want_n = 0.0, 0
    ring, h0, h1 = E.cuboids_torch(b, a, rr)
    for i in range(63):
        for j in range(i + 1, 63):
            if rr[i] != rr[j] or not vis[i] or not vis[j]:
                continue
            iou, inter = E._pair_iou(ring[i], h0[i], h1[i], ring[j], h0[j], h1[j])
            want_v += float(inter); want_n += int(iou > thresh)
    assert abs(float(vol[0]) - want_v) <= 1e-12 * max(1.0, want_v) and int(pairs[0]) == want_n and want_n > 0


def test_overlap_pairs_through_cuboid_iou_torch():
    """the same pair IoU through the public restatement: row j of a two-row 'room' of extent 1 against row i"""
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    b, a = torch.from_numpy(g["rand:boxes"][:21]), torch.from_numpy(g["rand:angles"][:21])
    rr = torch.from_numpy(g["rand:room_of_row"][:21])
    vis = torch.ones(21, dtype=torch.bool)
    _, _, pair_iou = E.layout_overlap_torch(b[None], a[None], rr, vis)
    ext = b[20, 3:6]
    scaled = torch.cat([b[:, :3].double() * ext.double(), b[:, 3:].double() * ext.double()], 1)
    unit = torch.tensor([[0, 0, 0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    k = 0
    for i in range(21):
        for j in range(i + 1, 21):
            iou, _ = E.cuboid_iou_torch(torch.cat([scaled[j:j + 1], unit])[None], torch.stack([a[j], a[20]])[None].double(),
                                        torch.cat([scaled[i:i + 1], unit]), torch.stack([a[i], a[20]]).double(), _rooms_of_single(2))
            assert abs(float(iou[0, 0]) - float(pair_iou[0, k])) < 1e-9, (i, j)
            k += 1
    assert k == pair_iou.shape[1] == 210


def test_room_rows_and_empty_mean():
    E = pkg("host.evaluate")
    objs = torch.tensor([3, 4, 0, 5, 0, 6])
    assert E.room_rows(objs, 0).tolist() == [2, 2, 2, 4, 4, -1]
    g = load_golden("refine_report")
    m = _meta(g)
    p = "hand:all_filtered:"
    objs = torch.from_numpy(g[p + "objs"])
    vis = E.visible_rows(objs, m["names"])
    assert not bool(vis.any())
    _, mean = E.cuboid_iou_torch(torch.from_numpy(g[p + "boxes"])[None], torch.from_numpy(g[p + "angles"])[None], torch.from_numpy(g[p + "gt_boxes"]),
                                 torch.from_numpy(g[p + "gt_angles"]), _rooms_of_single(len(objs)), vis)
    assert bool(torch.isnan(mean).all())                                    # np.mean([]) is nan
