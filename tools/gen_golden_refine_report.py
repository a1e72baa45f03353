"""Golden fixture for the refinement report (host/evaluate.py::cuboid_iou / layout_overlap, host/refine.py::RefineBatch(report=...)),
produced by EXECUTING THE REFERENCE'S OWN SOURCE TEXT (needs the reference tree; build container only).

``get_boxes`` and ``do_not_vis`` (testing/test_render_refine.py:16,78-116), ``get_eight_coors_bbox_new`` and ``get_iou_cuboid``
(testing/test_utils.py:7-40) and the ``for k in range(Niter_train)`` statement of ``finetune_VAE`` are taken out of the source text
with ``ast`` and ``exec``ed unmodified (``_top_level`` / ``_k_loop`` / ``reference_namespaces`` of oracle/gen_golden_refine.py).

What is injected (and therefore NOT pinned by this fixture):
  * ``Polygon`` - shapely is not installed: a stand-in with ``.area`` and ``.intersection(other).area`` for convex rings, written
    below in float64 (Sutherland-Hodgman + shoelace on python floats, unsigned areas, any winding, zero for degenerate rings).  It is
    the ONE restated piece, as the rasterizer ``nr`` is for the loop fixtures;
  * ``np`` inside ``get_boxes``: numpy >= 1.24 refuses the ragged ``np.array([corner, corner, corner, corner, h0, h1])`` the reference
    builds (:111-114); the stand-in's ``array`` falls back to ``dtype=object`` (what numpy did when the reference was written);
  * ``suncg_valid_types`` is the fixture's class-name list; everything oracle/gen_golden_refine.py injects for the loop.

Recorded:
  * the ``refine_loop`` and ``refine_loop_recurrent`` cases again (same state - read from the committed fixtures -, seeds and rooms),
    with a ``_record()`` that also evaluates, with the namespace's own ``matching_loss_func`` / ``ce_loss_func``, ``depth_mse`` and
    ``cross_entropy`` as :371-372 does, and the IoU of ``get_boxes(objs, boxes_gt, angles.float())`` against
    ``get_boxes(objs, boxes_pred, angles_pred_idx2)`` (the commented-out block :360-368).  Self-checks: what the reference itself
    pickles at k = 0 (:373) equals the k = 0 record; ``boxes`` / ``idx`` / ``loss`` equal the committed refine_loop*.npz bit for bit;
  * hand cases and 2 000 random pairs through the executed ``get_boxes`` + ``get_iou_cuboid``.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_refine_report.py

Writes tests/golden/refine_report.npz (numeric arrays + a json blob of names).
"""
import ast
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from oracle.gen_golden_refine import (GOLD, LOOP_CASES, LOOP_IMAGE, REF, VOCAB, _k_loop, _neutralise, _quiet, _room_graph, _run,      # noqa: E402
                                      _top_level, reference_namespaces, synth_tables)

NAMES = ["__room__"] + list(VOCAB)


# ------------------------------------------------------------------------------------------------------------------------------
# the stand-in for shapely.geometry.polygon.Polygon (float64, convex rings)
# ------------------------------------------------------------------------------------------------------------------------------
def _signed_area(pts):
    return 0.5 * sum(pts[i][0] * pts[(i + 1) % len(pts)][1] - pts[(i + 1) % len(pts)][0] * pts[i][1] for i in range(len(pts)))


class Polygon:
    def __init__(self, pts):
        self.pts = [(float(p[0]), float(p[1])) for p in pts]
        if len(self.pts) >= 3 and _signed_area(self.pts) < 0:
            self.pts = self.pts[::-1]

    @property
    def area(self):
        return abs(_signed_area(self.pts)) if len(self.pts) >= 3 else 0.0

    def intersection(self, other):
        poly, clip = list(self.pts), other.pts
        if self.area == 0.0 or other.area == 0.0:
            return Polygon([])
        for i in range(len(clip)):
            (bx, by), (cx, cy) = clip[i], clip[(i + 1) % len(clip)]
            side = lambda p: (cx - bx) * (p[1] - by) - (cy - by) * (p[0] - bx)
            out = []
            for k in range(len(poly)):
                cur, nxt = poly[k], poly[(k + 1) % len(poly)]
                dc, dn = side(cur), side(nxt)
                if dc >= 0:
                    out.append(cur)
                if (dc >= 0) != (dn >= 0):
                    t = dc / (dc - dn)
                    out.append((cur[0] + t * (nxt[0] - cur[0]), cur[1] + t * (nxt[1] - cur[1])))
            poly = out
            if not poly:
                break
        return Polygon(poly)


class _Numpy:
    """numpy whose ``array`` accepts the ragged list of get_boxes (:111-114) as an object array"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(x, *a, **k):
        try:
            return np.array(x, *a, **k)
        except ValueError:
            return np.array(x, dtype=object)


def iou_namespace():
    """-> namespace holding the executed get_boxes / get_eight_coors_bbox_new / get_iou_cuboid / do_not_vis"""
    _neutralise()
    tr_path, tu_path = os.path.join(REF, "testing/test_render_refine.py"), os.path.join(REF, "testing/test_utils.py")
    ns = dict(torch=torch, np=_Numpy(), Polygon=Polygon, suncg_valid_types=list(NAMES))
    _run(_top_level(tu_path, ["get_eight_coors_bbox_new", "get_iou_cuboid"]).values(), ns, tu_path)
    _run(_top_level(tr_path, ["do_not_vis", "get_boxes"]).values(), ns, tr_path)
    return ns


def reference_ious(ns, objs, gt_boxes, gt_angles, boxes, angles):
    """the print_iou block (:360-368) -> (iou of every kept row, the kept rows)"""
    objs_t = torch.as_tensor(objs)
    orig = ns["get_boxes"](objs_t, torch.as_tensor(gt_boxes), torch.as_tensor(gt_angles).float())
    cur = ns["get_boxes"](objs_t, torch.as_tensor(boxes), torch.as_tensor(angles))
    kept = [i for i in range(len(objs)) if NAMES[int(objs[i])] not in ns["do_not_vis"]]
    assert len(orig) == len(cur) == len(kept)
    return np.asarray([float(ns["get_iou_cuboid"](orig[i], cur[i])) for i in range(len(orig))], np.float64), np.asarray(kept, np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
# hand cases and random pairs
# ------------------------------------------------------------------------------------------------------------------------------
def hand_cases():
    """name -> (objs, gt_boxes, gt_angles, boxes, angles); room row last"""
    c = lambda n: NAMES.index(n)
    cube, slab = [0, 0, 0, 2.0, 2.0, 2.0], [0, 0, 0, 4.0, 2.5, 6.0]
    sq = [0.2, 0.0, 0.2, 0.4, 0.3, 0.4]                       # a square footprint
    cases = {}

    def add(name, objs, gt, ga, b, a):
        cases[name] = (np.asarray(objs, np.int64), np.asarray(gt, np.float32), np.asarray(ga, np.float32), np.asarray(b, np.float32),
                       np.asarray(a, np.float32))
    add("identical", [c("bed"), c("chair"), 0], [sq, [0.5, 0.1, 0.1, 0.9, 0.6, 0.3], cube], [0, 7, 0], [sq, [0.5, 0.1, 0.1, 0.9, 0.6, 0.3], cube], [0, 7, 0])
    add("disjoint", [c("bed"), 0], [sq, cube], [0, 0], [[0.6, 0.0, 0.6, 0.8, 0.3, 0.8], cube], [5, 0])
    add("inside", [c("sofa"), 0], [[0.1, 0.0, 0.1, 0.7, 0.6, 0.7], cube], [0, 0], [[0.3, 0.1, 0.3, 0.5, 0.4, 0.5], cube], [0, 0])
    add("heights_touch", [c("table"), 0], [sq, cube], [2, 0], [[0.2, 0.3, 0.2, 0.4, 0.5, 0.4], cube], [2, 0])
    add("octagon", [c("desk"), 0], [sq, cube], [0, 0], [sq, cube], [3, 0])
    add("bins", [c("bed"), c("chair"), c("sofa"), c("table"), c("desk"), c("lamp"), 0],
        [[0.1, 0, 0.1, 0.5, 0.3, 0.3]] * 6 + [slab], [0, 0, 0, 0, 0, 0, 0],
        [[0.12, 0.02, 0.1, 0.5, 0.3, 0.33]] * 6 + [slab], [0, 6, 12, 23, 2.37, -0.81, 0])
    add("flipped", [c("bed"), c("chair"), c("sofa"), c("table"), 0],
        [[0.1, 0.05, 0.2, 0.5, 0.4, 0.45]] * 4 + [slab], [1, 1, 1, 1, 0],
        [[0.55, 0.05, 0.2, 0.15, 0.4, 0.5], [0.15, 0.05, 0.5, 0.55, 0.4, 0.2], [0.55, 0.05, 0.5, 0.15, 0.4, 0.2], [0.15, 0.4, 0.2, 0.55, 0.05, 0.5], slab],
        [2.5, 0.5, 1.5, 1, 0])
    add("zero_width", [c("bed"), c("chair"), c("sofa"), 0],
        [sq, [0.2, 0, 0.2, 0.2, 0.3, 0.4], [0.2, 0, 0.2, 0.2, 0.3, 0.2], cube], [0, 3, 0, 0],
        [[0.3, 0, 0.2, 0.3, 0.3, 0.4], [0.2, 0, 0.2, 0.2, 0.3, 0.4], sq, cube], [4, 3, 0, 0])
    add("filtered", [c("bed"), c("door"), c("chair"), c("window"), 0],
        [sq, [0.0, 0, 0.4, 0.05, 0.8, 0.6], [0.5, 0, 0.5, 0.7, 0.4, 0.7], [0.3, 0.3, 0.0, 0.6, 0.7, 0.02], slab], [3, 0, 9, 0, 0],
        [[0.22, 0.01, 0.18, 0.43, 0.3, 0.41], [0.0, 0, 0.4, 0.05, 0.8, 0.6], [0.45, 0, 0.52, 0.7, 0.42, 0.66], [0.3, 0.3, 0.0, 0.6, 0.7, 0.02], slab],
        [3.4, 0, 10.2, 0, 0])
    add("all_filtered", [c("door"), c("window")], [[0.0, 0, 0.4, 0.05, 0.8, 0.6], [0.3, 0.3, 0.0, 0.6, 0.7, 0.02]], [0, 0],
        [[0.0, 0, 0.4, 0.05, 0.8, 0.6], [0.3, 0.3, 0.0, 0.6, 0.7, 0.02]], [0, 0])
    return cases


def random_rooms(n_rooms=100, per_room=20, seed=20240521):
    """2 000 (ground truth, prediction) pairs in the decoder's output range: room-normalised boxes in [0, 1] with x1 < x0 / z1 < z0 now
    and then, fractional angle bins in [-1, 24), room extents that are no cubes; the room row is predicted exactly (:300)"""
    rng = np.random.default_rng(seed)
    vis = [i for i, n in enumerate(NAMES) if n not in ("door", "window", "__room__")]
    objs, gt, ga, bp, ap, rr = [], [], [], [], [], []
    for r in range(n_rooms):
        ext = rng.uniform([2.0, 2.2, 2.0], [7.0, 3.2, 7.0])
        size = rng.uniform(0.05, 0.45, size=(per_room, 3))
        lo = rng.uniform(0.0, 1.0 - size)
        g = np.concatenate([lo, lo + size], 1)
        p = g + rng.normal(0, 0.05, size=g.shape) * (rng.random((per_room, 1)) < 0.85)
        far = rng.random(per_room) < 0.1
        p[far] = np.concatenate([lo[far][:, ::-1], lo[far][:, ::-1] + size[far]], 1)
        flip = rng.random(per_room) < 0.1
        p[flip] = p[flip][:, [3, 1, 2, 0, 4, 5]]
        flip = rng.random(per_room) < 0.1
        p[flip] = p[flip][:, [0, 1, 5, 3, 4, 2]]
        a_g = rng.integers(0, 24, size=per_room).astype(np.float64)
        a_p = np.where(rng.random(per_room) < 0.2, rng.uniform(-1, 24, size=per_room), a_g + rng.normal(0, 0.6, size=per_room))
        room = [0, 0, 0, ext[0], ext[1], ext[2]]
        base = r * (per_room + 1)
        objs += list(rng.choice(vis, size=per_room)) + [0]
        gt += g.tolist() + [room]; bp += p.tolist() + [room]
        ga += a_g.tolist() + [0.0]; ap += a_p.tolist() + [0.0]
        rr += [base + per_room] * (per_room + 1)
    return (np.asarray(objs, np.int64), np.asarray(gt, np.float32), np.asarray(ga, np.float32), np.asarray(bp, np.float32), np.asarray(ap, np.float32),
            np.asarray(rr, np.int32))


# ------------------------------------------------------------------------------------------------------------------------------
# the loops again, with the report
# ------------------------------------------------------------------------------------------------------------------------------
def gen_loop_case(case, ins, out):
    from oracle import gen_golden, vae_ref
    cfg_kw, rooms, iters = LOOP_CASES[case]
    committed = np.load(os.path.join(GOLD, case + ".npz"))
    tables = synth_tables()
    _, ref_vae, _ = gen_golden._import_reference()
    cfg = vae_ref.VaeConfig(**cfg_kw)
    sd0 = {k[len("state:"):]: torch.from_numpy(committed[k]) for k in committed.files if k.startswith("state:")}
    for r, (seed, n_obj) in enumerate(rooms):
        ns, ns2 = reference_namespaces(tables, LOOP_IMAGE)
        objs_np, tri, boxes_np, angles_np, attrs_np = _room_graph(cfg, seed, n_obj)
        n = n_obj + 1
        model = ref_vae.Sg2ScVAEModel(**cfg.model_kwargs())
        model.load_state_dict({k_: v_.clone() for k_, v_ in sd0.items()})
        model.eval()
        objs, triples, boxes_gt, angles, attributes = (torch.from_numpy(a) for a in (objs_np, tri, boxes_np, angles_np, attrs_np))
        p = "room%d:" % r
        z_np = committed[p + "z0"].copy()
        mu, logvar = model.encoder(objs, triples, boxes_gt, angles, attributes)
        torch.manual_seed(13)
        z_again = (mu + torch.randn_like(mu) * torch.exp(0.5 * logvar)).detach().numpy()     # (leaves the generator where the loop expects it)
        assert np.array_equal(z_again, z_np), "z0 differs from the committed fixture"
        rec, dumped = [], []
        env = dict(ns2)
        del env["_finetune_node"]

        def _record():
            e = env
            depth_mse = e["matching_loss_func"](e["iter_image"][:, 41:], e["target"][:, 41:])
            cross_entropy = e["ce_loss_func"](e["train_labels_pooled"][-1], e["target_container"][-1][:, 0, :, :].type(torch.LongTensor))
            ious, kept = reference_ious(ins, objs_np, boxes_gt, angles, e["boxes_pred"].detach(), e["angles_pred_idx2"].detach())
            rec.append(dict(loss=float(e["loss_val"].detach()), boxes=e["boxes_pred"].detach().clone().numpy(),
                            idx=e["angles_pred_idx2"].detach().clone().numpy(), depth_mse=float(depth_mse.item()),
                            cross_entropy=float(cross_entropy.item()), ious=ious, kept=kept, iou=float(np.mean(ious))))

        def _dump(obj, f):
            dumped.append(obj)
        env.update(model=model, z=None, z_np=z_np.copy(), save_name=tempfile.mkdtemp(prefix="sln_refine_report_"),
                   float_dtype=torch.FloatTensor, long_dtype=torch.LongTensor,
                   args=types.SimpleNamespace(learning_rate=1e-4), objs=objs, triples=triples, attributes=attributes,
                   obj_to_img=torch.zeros(n, dtype=torch.int64), boxes_gt=boxes_gt, angles=angles, mesh_render_func=ns["mesh_render_func"],
                   save_images=_quiet, pickle=types.SimpleNamespace(dump=_dump), target_mesh=None, model_infos=None, size_infos=None,
                   Niter_train=iters, used_ids=[r], trial=0, orig_bbox=None, _record=_record)
        exec(compile(ast.Module(body=[_k_loop(ns2["_finetune_node"])], type_ignores=[]), "testing/test_render_refine.py", "exec"), env)
        assert len(rec) == iters
        # the same loop as the committed fixture's, bit for bit
        assert np.array_equal(np.stack([x["boxes"] for x in rec]), committed[p + "boxes"]), "boxes differ from " + case
        assert np.array_equal(np.stack([x["idx"] for x in rec]), committed[p + "idx"]), "idx differ from " + case
        assert np.array_equal(np.asarray([x["loss"] for x in rec], np.float64), committed[p + "loss"]), "loss differs from " + case
        # what the reference itself dumps at k = 0 (:373): [id, boxes, angles, size_infos, model_infos, depth_mse, cross_entropy]
        d0 = [d for d in dumped if isinstance(d, list) and len(d) == 7]          # (the other dumps: z_value.pkl, bbox_rot_gt_0.pkl)
        assert len(d0) == 1 and d0[0][5] == rec[0]["depth_mse"] and d0[0][6] == rec[0]["cross_entropy"], "k = 0 dump differs from the record"
        assert np.array_equal(np.stack(d0[0][1]), rec[0]["boxes"]) and np.array_equal(np.stack(d0[0][2]), rec[0]["idx"])
        q = "loop:%s:room%d:" % (case, r)
        for k_ in ("iou", "depth_mse", "cross_entropy"):
            out[q + k_] = np.asarray([x[k_] for x in rec], np.float64)
        out[q + "ious"] = np.stack([x["ious"] for x in rec])
        out[q + "kept"] = rec[0]["kept"]
        print("%s room %d: iou %s depth_mse %s ce %s" % (case, r, ["%.4f" % x["iou"] for x in rec], ["%.5f" % x["depth_mse"] for x in rec],
                                                         ["%.4f" % x["cross_entropy"] for x in rec]))


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    ins = iou_namespace()
    out = {}
    cases = hand_cases()
    for name, (objs, gt, ga, b, a) in cases.items():
        ious, kept = reference_ious(ins, objs, gt, ga, b, a)
        for k_, v_ in (("objs", objs), ("gt_boxes", gt), ("gt_angles", ga), ("boxes", b), ("angles", a), ("iou", ious), ("kept", kept)):
            out["hand:%s:%s" % (name, k_)] = v_
        print("hand %-14s %s" % (name, " ".join("%.6f" % x for x in ious)))
    objs, gt, ga, b, a, rr = random_rooms()
    ious = np.full(len(objs), np.nan)
    for r0 in sorted(set(rr.tolist())):
        rows = np.nonzero(rr == r0)[0]
        v, kept = reference_ious(ins, objs[rows], gt[rows], ga[rows], b[rows], a[rows])
        assert len(kept) == len(rows)
        ious[rows] = v
    for k_, v_ in (("objs", objs), ("gt_boxes", gt), ("gt_angles", ga), ("boxes", b), ("angles", a), ("room_of_row", rr), ("iou", ious)):
        out["rand:" + k_] = v_
    print("random pairs: %d rows, mean iou %.4f, %d zero" % (len(ious), ious.mean(), int((ious == 0).sum())))
    for case in LOOP_CASES:
        gen_loop_case(case, ins, out)
    out["meta"] = np.frombuffer(json.dumps(dict(names=NAMES, do_not_vis=list(ins["do_not_vis"]), hand=list(cases), loops={
        c: len(LOOP_CASES[c][1]) for c in LOOP_CASES})).encode(), dtype=np.uint8)
    path = os.path.join(GOLD, "refine_report.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
