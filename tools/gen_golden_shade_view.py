"""Golden fixture for the viewpoint render (host/shade.py, csrc/shade_view.hip), produced by EXECUTING THE REFERENCE'S OWN SOURCE TEXT
(needs the reference tree; build container only).

Statements of ``render_test`` (render/render_semantic_depth.py) are taken out of the source text with ``ast`` and ``exec``ed unmodified -
the module itself cannot be imported (it needs ``bpy``):

  :153-173    box restoration (un-normalising by the room row, the ``abs(y0) <= 0.02`` height adjustment, ``room_bbox``)
  :202-234    the object transform (``scale``, ``theta``, ``rot``, the bottom-resting ``obj_center[1]``, ``trans``)
  :240        the class list that is not imported (the literal of the comparison)
  :350-377    the viewpoint statements and the acceptance loop, as ONE ``for`` statement

What is injected (and therefore NOT pinned): ``suncg_data`` / ``object_idx_to_name`` / ``ids`` are the small tables below, ``np`` is a
namespace that forwards to numpy with ``random.rand`` replaying recorded draws, ``camera`` is a stand-in whose ``add_camera`` records its
arguments and whose ``get_camera_zbuffer`` hands out the next synthetic z-buffer (float64 arrays), ``scene`` is an empty namespace.
Blender itself - its OBJ importer's axes, its clipping at ``clip_start``, Cycles' mask edges - is not run and not pinned.

The acceptance loop runs over synthetic z-buffers whose sums are exact in any order: a mean exactly at 0.7 (sum 7 over 10 entries: not
accepted, ``>`` is strict), no accepted view, a first and second view that fail and a third that passes, entries at and above 1e5, and a
second time with the literal 0.7 of :375 replaced by the name ``threshold`` (the only edit; 0.75 = 6 / 8 is exactly representable).  It
also runs over the z-buffers ``views_torch`` (float64, the C restatement of the rasterizer) renders of one golden room, whose first two
viewpoints face a tall cabinet (the camera stands 0.4 m outside the room and looks down: no object brings a mean below 0.7, so this run
uses the threshold parameter, 2.0, and records the unmodified loop's choice next to it): the recorded choice is what ``tests/test_shade_view_host.py`` holds ``views_torch`` to.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_shade_view.py

Writes tests/golden/shade_view.npz (numeric arrays only; member times are fixed, so the file regenerates bit for bit).
"""
import ast
import copy
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from oracle.gen_golden_refine import GOLD, REF, _run, _top_level      # noqa: E402
from tools.gen_golden_mesh_retrieve import write_npz                   # noqa: E402

SRC = os.path.join(REF, "render/render_semantic_depth.py")
VOCAB = ["__room__", "bed", "chair", "desk", "door", "window", "lamp", "cabinet"]
VIEW_S = 32                     # image size of the rendered golden room


def _body(lo, hi):
    """the statements of render_test's body whose first line lies in [lo, hi]"""
    fn = _top_level(SRC, ["render_test"])["render_test"]
    return [n for n in fn.body if lo <= n.lineno <= hi]


def _not_imported():
    loop = _body(238, 238)
    assert len(loop) == 1 and isinstance(loop[0], ast.For)
    test = loop[0].body[1].test
    assert isinstance(test, ast.Compare) and isinstance(test.ops[0], ast.In) and test.lineno == 240
    return list(ast.literal_eval(test.comparators[0]))


def tables(rng):
    data = {}
    for name in VOCAB[1:]:
        data[name] = []
        for k in range(int(rng.integers(1, 4))):
            lo = rng.uniform(-1.0, 0.5, size=3).astype(np.float32).astype(np.float64)
            size = rng.uniform(0.3, 2.0, size=3).astype(np.float32).astype(np.float64)
            data[name].append({"id": "%s_%d" % (name, k), "bbox_min": [float(x) for x in lo], "bbox_max": [float(x) for x in (lo + size).astype(np.float32)]})
    return data


def rooms(rng):
    """[(objs, boxes float64 [n, 6] of float32 values, angles)] with the room row last.  Shallow rooms: the viewpoint looks down by about
    54 degrees, so the centre of the back wall is inside the picture only where atan(0.4 h / (z + 0.4)) exceeds the top ray's depression
    (asserted by the host test from plain trigonometry)"""
    out = []
    for r in range(7):
        n = int(rng.integers(2, 9))
        objs = [int(x) for x in rng.integers(1, len(VOCAB), size=n)] + [0]
        lo = rng.uniform(0.0, 0.6, size=(n, 3))
        lo[:, 1] = rng.choice([0.0, 0.004, -0.005, 0.3], size=n) if r != 3 else 0.0
        b = np.concatenate([lo, lo + rng.uniform(0.05, 0.4, size=(n, 3))], 1)
        ext = rng.uniform([2.0, 2.6, 1.0], [4.0, 3.2, 1.6])
        org = np.zeros(3) if r % 3 else rng.uniform(0.0, 0.3, size=3)
        room = np.concatenate([org, org + ext])
        boxes = np.concatenate([b, room[None]]).astype(np.float32)
        if r == 3:          # the height adjustment's threshold from both sides: y0 * ext_y at, just below and just above 0.02
            e = np.float64(boxes[-1, 4]) - np.float64(boxes[-1, 1])
            for i, target in enumerate([0.02, 0.0199, 0.0201, -0.02][:n]):
                boxes[i, 1] = np.float32(target / e)
        ang = rng.integers(0, 24, size=n + 1).astype(np.float64)
        if r % 2:
            ang[:-1] += rng.uniform(-0.5, 0.5, size=n).astype(np.float32)
        out.append((objs, boxes.astype(np.float64), ang))
    return out


def _numpy_with_draws(draws):
    ns = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    it = iter(draws)
    ns.random = types.SimpleNamespace(rand=lambda: float(next(it)))
    return ns


class _Camera:
    """stands in for render/blender_util's ``camera``: records the viewpoints, hands out the z-buffers"""

    def __init__(self, zbuffers):
        self.z, self.added = list(zbuffers), []

    def add_camera(self, xyz, rot_vec_rad, f, sensor_width, sensor_height, sensor_fit):
        assert (sensor_width, sensor_height, sensor_fit) == (50, 50, 'VERTICAL') and rot_vec_rad[2] == 0
        self.added.append((np.array(xyz, dtype=np.float64), -float(rot_vec_rad[0]), float(rot_vec_rad[1]), float(f)))
        return len(self.added) - 1

    def get_camera_zbuffer(self, cam):
        return self.z[cam]


def run_views(room_bbox, draws, zbuffers, threshold=None):
    """:350-377 -> (chosen view or -1, the recorded viewpoints)"""
    nodes = copy.deepcopy(_body(350, 353))
    assert len(nodes) == 3 and isinstance(nodes[2], ast.For) and nodes[2].end_lineno == 377
    ns = dict(np=_numpy_with_draws(np.asarray(draws).reshape(-1)), camera=_Camera(zbuffers), scene=types.SimpleNamespace(), room_bbox=room_bbox)
    if threshold is not None:
        hits = [n for n in ast.walk(nodes[2]) if isinstance(n, ast.Compare) and isinstance(n.comparators[0], ast.Constant) and n.comparators[0].value == 0.7]
        assert len(hits) == 1 and hits[0].lineno == 375
        hits[0].comparators[0] = ast.copy_location(ast.Name(id="threshold", ctx=ast.Load()), hits[0].comparators[0])
        ns["threshold"] = threshold
    _run(nodes, ns, SRC)
    return (int(ns["k"]) if ns["succeed"] else -1), ns["camera"].added


def run_placement(objs, boxes, angles, data, model_of_row):
    ns = dict(np=np, copy=copy, suncg_data=data, object_idx_to_name=list(VOCAB), dataset="suncg", objs=list(objs), angles=[float(a) for a in angles],
              boxes=[[float(x) for x in row] for row in boxes])
    ns["ids"] = [data[VOCAB[c]][k]["id"] for c, k in zip(objs[:-1], model_of_row)]
    _run(_body(153, 173) + _body(202, 206), ns, SRC)
    return ns


def acceptance_cases():
    """[(name, threshold or None, z-buffers [5, 4, 4])]; every entry a multiple of 1 / 8, every sum exact"""
    far = 1e10

    def zb(values):
        z = np.full(16, far)
        z[:len(values)] = values
        return z.reshape(4, 4)
    at = zb([0.5] * 6 + [1.0] * 4)                      # sum 7, 10 entries: exactly the double 0.7
    above = zb([0.5] * 6 + [1.0] * 3 + [1.125])
    low = zb([0.25] * 16)
    high = zb([2.0] * 16)
    edge = zb([0.5] * 4 + [1e5, 2e5, 1e5 + 1.0])        # at and above 1e5: not summed (summed, they would carry the view over the threshold)
    q = zb([0.75] * 8)
    cases = [("at_threshold_then_above", None, [at, at, above, high, high]), ("none_accepted", None, [low, at, low, at, low]),
             ("third_passes", None, [low, at, high, high, low]), ("first_passes", None, [high, low, low, low, low]),
             ("last_passes", None, [low, low, low, low, above]), ("at_1e5", None, [low, edge, high, low, low]),
             ("param_at_threshold", 0.75, [q, q, q, q, q]), ("param_above", 0.75, [q, zb([0.75] * 7 + [0.875]), q, q, q]),
             ("param_half", 0.5, [zb([0.5] * 16), zb([0.5] * 15 + [0.625]), high, high, high])]
    return [(n, t, np.stack(z)) for n, t, z in cases]


def view_room():
    """one golden room whose first two viewpoints stand in front of a tall cabinet by the front wall"""
    sizes = np.array([[1.0, 2.0, 0.5], [0.8, 0.5, 0.8]], dtype=np.float32)                   # cabinet, bed (models: cuboids of these sizes)
    boxes = np.array([[0.02, 0.0, 0.70, 0.55, 0.93, 0.98], [0.60, 0.0, 0.20, 0.90, 0.20, 0.60], [0, 0, 0, 3.0, 2.8, 1.5]], dtype=np.float32)
    objs = np.array([VOCAB.index("cabinet"), VOCAB.index("bed"), 0], dtype=np.int64)
    angles = np.array([0.0, 3.0, 0.0], dtype=np.float32)
    draws = np.array([[[0.05, 0.5], [0.15, 0.9], [0.95, 0.25], [0.9, 0.0], [0.5, 0.5]]], dtype=np.float32)
    return sizes, boxes, objs, angles, draws


def view_bank(RF, syn, sizes, device="cpu"):
    meshes = {}
    for name, size in zip(("cabinet", "bed"), sizes):
        v, f = syn._grid_cuboid(-np.asarray(size, np.float64) / 2, np.asarray(size, np.float64) / 2, 2)
        meshes[name] = (v.astype(np.float32), f.astype(np.int32))
    return RF.MeshBank.from_arrays(meshes, device, vocab=VOCAB[1:])


def main(path=None):
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    SH, RF, syn = (importlib.import_module("3d_sln_amd.host." + m) for m in ("shade", "refine", "synthetic"))
    from oracle import raster_ref
    rng = np.random.default_rng(20261)
    data = tables(rng)
    out = dict(vocab=np.frombuffer("\n".join(VOCAB).encode(), dtype=np.uint8),
               not_imported=np.frombuffer("\n".join(_not_imported()).encode(), dtype=np.uint8))
    flat = [(ci, e) for ci, c in enumerate(VOCAB) for e in data.get(c, [])]
    first = {ci: next(k for k, (cj, _) in enumerate(flat) if cj == ci) for ci in range(1, len(VOCAB))}
    out["model_class"] = np.asarray([ci for ci, _ in flat], np.int32)
    out["model_bbox"] = np.asarray([[e["bbox_min"], e["bbox_max"]] for _, e in flat], np.float64)
    objs_all, boxes_all, ang_all, room_row, row_model, A, tr, center, scaled, restored, snapped = [], [], [], [], [], [], [], [], [], [], 0
    cams, draws_all, row0 = [], [], 0
    for objs, boxes, ang in rooms(rng):
        n = len(objs)
        pick = [int(rng.integers(0, len(data[VOCAB[c]]))) for c in objs[:-1]]
        ns = run_placement(objs, boxes, ang, data, pick)
        assert len(ns["rotations"]) == n - 1
        snapped += sum(1 for i in range(n - 1) if ns["boxes"][i][1] == 0 and boxes[i][1] != 0)
        pad3, pad33 = np.full(3, np.nan), np.full((3, 3), np.nan)
        A += [np.asarray(x) for x in ns["rotations"]] + [pad33]; tr += [np.asarray(x) for x in ns["translations"]] + [pad3]
        center += [np.asarray(x) for x in ns["centers"]] + [pad3]; scaled += [np.asarray(x) for x in ns["sizes"]] + [pad3]
        restored.append(np.asarray(ns["boxes"], dtype=np.float64))
        objs_all += objs; boxes_all.append(boxes); ang_all.append(ang); room_row += [row0 + n - 1] * n
        row_model += [first[c] + k for c, k in zip(objs[:-1], pick)] + [-1]; row0 += n
        # the viewpoints of this room (:355-360): five recorded draws; z-buffers that are never accepted, so that all five are formed
        draws = rng.uniform(size=(5, 2))
        draws[0] = (0.0, 0.0) if len(cams) == 0 else draws[0]
        chosen, added = run_views(ns["room_bbox"], draws, [np.full((2, 2), 0.5)] * 5)
        assert chosen == -1 and len(added) == 5 and all(a[3] == 50 for a in added)
        cams.append(added); draws_all.append(draws)
    out.update(objs=np.asarray(objs_all, np.int32), boxes=np.concatenate(boxes_all), angles=np.concatenate(ang_all), room_row=np.asarray(room_row, np.int32),
               row_model=np.asarray(row_model, np.int32), A=np.stack(A), tr=np.stack(tr), center=np.stack(center), scaled_size=np.stack(scaled),
               restored=np.concatenate(restored), draws=np.stack(draws_all),
               cam_coord=np.stack([[a[0] for a in c] for c in cams]), canonical_angle=np.asarray([[a[1] for a in c] for c in cams]),
               plane_angle=np.asarray([[a[2] for a in c] for c in cams]))
    assert snapped >= 6, snapped
    # the acceptance loop over synthetic z-buffers
    names, thr, zs, chosen = [], [], [], []
    ext = [3.0, 2.8, 1.5]
    for name, t, z in acceptance_cases():
        k, _ = run_views(ext, np.zeros(10), list(z), threshold=t)
        names.append(name); thr.append(np.nan if t is None else t); zs.append(z); chosen.append(k)
    want = dict(at_threshold_then_above=2, none_accepted=-1, third_passes=2, first_passes=0, last_passes=4, at_1e5=2, param_at_threshold=-1,
                param_above=1, param_half=1)
    assert dict(zip(names, chosen)) == want, dict(zip(names, chosen))
    out.update(accept_names=np.frombuffer("\n".join(names).encode(), dtype=np.uint8), accept_threshold=np.asarray(thr), accept_z=np.stack(zs),
               accept_chosen=np.asarray(chosen, np.int32))
    # the restatements against what the reference computed, before anything is written
    T = torch.from_numpy
    pl = SH.shade_placement(T(out["boxes"]), T(out["angles"]), T(out["row_model"]).clamp(min=0), T(out["room_row"]), T(out["model_bbox"]))
    obj = out["row_model"] >= 0
    for key in ("A", "tr", "center", "scaled_size"):
        assert np.array_equal(pl[key].numpy()[obj], out[key][obj]), key
    assert np.array_equal(pl["boxes"].numpy()[obj], out["restored"][obj])
    last = np.unique(out["room_row"])
    room = out["boxes"][last]
    cam, can, pla = SH.shade_viewpoint(T(room[:, 3:] - room[:, :3])[:, None, :].expand(-1, 5, 3), T(out["draws"][..., 0]), T(out["draws"][..., 1]))
    assert np.array_equal(cam.numpy(), out["cam_coord"]) and np.array_equal(can.numpy(), out["canonical_angle"]) and np.array_equal(pla.numpy(), out["plane_angle"])
    # one golden room through views_torch: its z-buffers into the reference's loop
    sizes, boxes, objs, angles, draws = view_room()
    bank = view_bank(RF, syn, sizes)
    thr = 2.0                   # between the means of the two views that face the cabinet and those of the three that do not
    got = SH.views_torch(bank, T(boxes).double(), T(angles).double(), T(objs), [3], T(draws), raster_ref.nmr_forward, size=VIEW_S, vocab=VOCAB,
                         min_mean_depth=thr)
    z = got["depth_all"].double().numpy()
    k, _ = run_views([3.0, 2.8, 1.5], draws.astype(np.float64), list(z), threshold=thr)
    k07, _ = run_views([3.0, 2.8, 1.5], draws.astype(np.float64), list(z))
    means = (got["sums"] / got["counts"].clamp(min=1)).numpy()
    print("golden room: means %s, the reference's loop chose view %d (%d at 0.7), views_torch %d" % (np.round(means, 4), k, k07, int(got["chosen"][0])))
    assert k == 2 and k07 == 0 and int(got["chosen"][0]) == 2 and int(got["status"][0]) == 0 and (np.abs(means - thr) > 0.05).all()
    out.update(view_sizes=sizes, view_boxes=boxes, view_objs=objs.astype(np.int32), view_angles=angles, view_draws=draws,
               view_chosen=np.asarray([k, k07], np.int32), view_threshold=np.asarray([thr, 0.7]), view_means=means, view_S=np.asarray([VIEW_S], np.int32))
    path = path or os.path.join(GOLD, "shade_view.npz")
    write_npz(path, out)
    print("wrote %s: %d arrays, %d bytes; %d rows, %d snapped heights" % (path, len(out), os.path.getsize(path), len(out["objs"]), snapped))
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
