"""Golden fixture for the 3-D drawing (host/draw3d.py, csrc/draw3d.hip), produced by EXECUTING THE REFERENCE'S OWN SOURCE TEXT (needs
the reference tree; build container only).  Statements are taken out of render/render_room_color.py and render/render_caller.py with
``ast`` and ``exec``ed unmodified - neither module can be imported (they need ``bpy``):

  * the ``lighting.add_light_area`` call of ``render_test`` under a recording stub, for four room extents: position, energy, size;
  * the three ``scene.render.resolution_*`` assignments in front of the viewpoint loop;
  * ``render_caller.py::render_test_3d`` for a two-room dict, with ``render_test`` a stub that records the ``name`` it is given;
  * three booleans: ``ast.dump`` of (a) the restore / snap / placement statements, (b) the shell block from ``walls = []`` up to the
    viewpoint loop and (c) the viewpoint loop equal those of render/render_semantic_depth.py::render_test.  Equality is what lets the
    3-D drawing rest on the pins of tests/golden/shade_view.npz.

What Blender does with the lamp, the resolution and the materials is not run and not pinned.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_draw3d.py

Writes tests/golden/draw3d.npz (numeric arrays only; member times are fixed, so the file regenerates bit for bit).
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from oracle.gen_golden_refine import GOLD, REF, _run, _top_level      # noqa: E402
from tools.gen_golden_mesh_retrieve import write_npz                   # noqa: E402

COLOR = os.path.join(REF, "render/render_room_color.py")
DEPTH = os.path.join(REF, "render/render_semantic_depth.py")
CALLER = os.path.join(REF, "render/render_caller.py")
EXTENTS = [[4.0, 2.7, 5.0], [3.1415927, 2.4000001, 2.0999999], [2.5, 3.2, 4.7], [3.0, 2.8, 1.5]]
ROOM_IDS = ["room_000", "bedroom_17"]


def _is_assign_to(node, name):
    return isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id == name


def blocks(path):
    """-> dict of statement lists of ``render_test``: placement (restore, snap, the transform loop), shell, views (the loop), and the
    statements between the shell's last import and the loop (``resolution``)"""
    body = _top_level(path, ["render_test"])["render_test"].body
    at = lambda pred: next(i for i, n in enumerate(body) if pred(n))
    room = at(lambda n: _is_assign_to(n, "room_bbox"))
    rot = at(lambda n: _is_assign_to(n, "rotations"))
    objs = at(lambda n: _is_assign_to(n, "room_objs"))
    walls = at(lambda n: _is_assign_to(n, "walls"))
    loop = at(lambda n: isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id == "k")
    assert 0 < room < rot < objs < walls < loop and isinstance(body[objs - 1], ast.For)
    res = [n for n in body[walls:loop] if isinstance(n, ast.Assign) and "resolution" in ast.dump(n.targets[0])]
    return dict(placement=body[:room + 1] + body[rot:objs], shell=body[walls:loop], views=[body[loop]], resolution=res, body=body)


def _dump(nodes):
    return "\n".join(ast.dump(n) for n in nodes)


def light_calls():
    """the ``add_light_area`` statement for every extent of EXTENTS -> [(xyz, energy, size)]"""
    stmts = [n for n in blocks(COLOR)["body"] if isinstance(n, ast.Assign) and "add_light_area" in ast.dump(n.value)]
    assert len(stmts) == 1
    seen = []

    def add_light_area(xyz, rot_vec_rad, name, energy, size):
        assert tuple(rot_vec_rad) == (0, 0, 0) and name is None
        seen.append((np.asarray(xyz, np.float64), float(energy), float(size)))
    for ext in EXTENTS:
        _run(stmts, dict(lighting=types.SimpleNamespace(add_light_area=add_light_area), room_bbox=[float(x) for x in ext]), COLOR)
    return seen


def resolution():
    scene = types.SimpleNamespace(render=types.SimpleNamespace())
    stmts = blocks(COLOR)["resolution"]
    assert len(stmts) == 3
    _run(stmts, dict(scene=scene), COLOR)
    return [scene.render.resolution_x, scene.render.resolution_y, scene.render.resolution_percentage]


def caller_names(data):
    """render_caller.py::render_test_3d on ``data`` -> the names it hands to ``render_test``, in order"""
    fn = _top_level(CALLER, ["render_test_3d"])["render_test_3d"]
    names = []

    def render_test(objs, boxes, angles, output_folder, name):
        names.append(name)
    path = types.SimpleNamespace(join=os.path.join, isdir=lambda p: True)
    ns = dict(os=types.SimpleNamespace(path=path, mkdir=lambda p: None), load_json=lambda p: data, render_test=render_test)
    _run([fn], ns, CALLER)
    ns["render_test_3d"]("somewhere")
    return names


def two_rooms():
    """a ``data_extracted.json``-shaped dict of two rooms (three and two rows; the room row last)"""
    data = {}
    for r, room_id in enumerate(ROOM_IDS):
        n = 2 - r
        objs = [1 + r, 3, 0][:n] + [0]
        room = {"gt": {"objs": objs}}
        for k in range(4):
            boxes = [[0.1 + 0.05 * k + 0.3 * i, 0.0, 0.2 + 0.2 * i, 0.35 + 0.05 * k + 0.3 * i, 0.25, 0.5 + 0.2 * i] for i in range(n)]
            room[str(k)] = {"boxes": boxes + [[0.0, 0.0, 0.0, 4.0 - r, 2.7, 3.0 + r]], "angles": [float((3 * k + i) % 24) for i in range(n)] + [0.0]}
        data[room_id] = room
    return data


def main(path=None):
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    color, depth = blocks(COLOR), blocks(DEPTH)
    lights = light_calls()
    names = caller_names(two_rooms())
    out = dict(extents=np.asarray(EXTENTS, np.float64), light_xyz=np.stack([x for x, _, _ in lights]),
               light_energy=np.asarray([e for _, e, _ in lights]), light_size=np.asarray([s for _, _, s in lights]),
               resolution=np.asarray(resolution(), np.int32), names=np.frombuffer("\n".join(names).encode(), dtype=np.uint8),
               same_geometry=np.asarray([_dump(color[k]) == _dump(depth[k]) for k in ("placement", "shell", "views")], np.bool_))
    assert len(names) == 8 and out["same_geometry"].all(), (names, out["same_geometry"])
    path = path or os.path.join(GOLD, "draw3d.npz")
    write_npz(path, out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 4096


if __name__ == "__main__":
    main()
