"""Cases shared by tests/test_shade_view_host.py and tests/test_shade_view_gpu.py: a small bank, rooms at the shapes where the face-slot
indexing of csrc/shade_view.hip can break, and the error metric the operand tests use."""
import numpy as np
import torch

from conftest import pkg

VOCAB = ["__room__", "bed", "chair", "desk", "lamp", "door", "alien"]       # door: not imported (:240); alien: no NYU class, no model
NEAR = 0.1
# (name, image size, rooms, views, near): R * V in {1, 5, 17} - 17 views take the rasterizer's batch route -, S in {8, 33, 64, 100}
CASES = [("one_view", 8, 1, 1, NEAR), ("five_views", 33, 1, 5, NEAR), ("seventeen_rooms", 64, 17, 1, NEAR), ("five_views_100", 100, 1, 5, NEAR),
         ("seventeen_views", 33, 1, 17, NEAR), ("no_visible_row", 33, 2, 1, NEAR), ("every_face_culled", 33, 1, 5, 50.0)]


def _cuboid(size, subdiv, shift=(0.0, 0.0, 0.0)):
    syn = pkg("host.synthetic")
    size, shift = np.asarray(size, np.float64), np.asarray(shift, np.float64)
    v, f = syn._grid_cuboid(-size / 2 + shift, size / 2 + shift, subdiv)
    return v.astype(np.float32), f.astype(np.int32)


def bank(device):
    """bed: one model of 12 faces; chair: two models (12 and 48 faces: the slot count is the larger) among which the retrieval picks;
    desk: 48 faces, off-centre; lamp: 108 faces; door: a model that is never imported"""
    RF = pkg("host.refine")
    meshes = {"bed": _cuboid((2.0, 0.5, 1.5), 1), "chair": [_cuboid((0.5, 1.0, 0.5), 1) + ([-0.25, -0.5, -0.25], [0.25, 0.5, 0.25], "chair_tall"),
                                                            _cuboid((1.0, 0.4, 1.0), 2) + ([-0.5, -0.2, -0.5], [0.5, 0.2, 0.5], "chair_flat")],
              "desk": _cuboid((1.4, 0.75, 0.7), 2, shift=(0.3, 0.1, -0.2)), "lamp": _cuboid((0.3, 1.5, 0.3), 3), "door": _cuboid((0.9, 2.0, 0.1), 1)}
    return RF.MeshBank.from_arrays(meshes, device, vocab=VOCAB[1:])


def case(name):
    """-> dict(S, R, V, near, boxes [n, 6] float32, angles [n] float32, objs [n] int64, rows, draws [R, V, 2] float32)"""
    _, S, R, V, near = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    boxes, angles, objs, rows = [], [], [], []
    for r in range(R):
        n = int(rng.integers(2, 7)) if R > 1 else 6                       # rooms of different lengths: the shorter ones are padded
        cls = rng.choice([1, 2, 3, 4, 5, 6], size=n, p=[0.2, 0.35, 0.15, 0.1, 0.1, 0.1])
        if R == 1:
            cls[:4] = [2, 2, 1, 2]                                       # a model used by two rows (and by a third, of another shape)
        if name == "no_visible_row":
            cls = np.full(n, 5) if r == 0 else cls[:0]                   # doors only; a room that is its room row alone
            n = len(cls)
        ext = rng.uniform([2.5, 2.4, 2.0], [5.0, 3.2, 4.5])
        lo = rng.uniform([0.05, 0.0, 0.05], [0.6, 0.3, 0.6], size=(n, 3))
        lo[:, 1] = rng.choice([0.0, 0.005, 0.2], size=n)
        b = np.concatenate([lo, lo + rng.uniform(0.1, 0.35, size=(n, 3))], 1)
        flat = rng.random(n) < 0.5
        b[flat, 4] = b[flat, 1] + 0.08                                    # low boxes: the flat chair
        boxes.append(np.concatenate([b, [[0, 0, 0, ext[0], ext[1], ext[2]]]]))
        angles.append(np.concatenate([rng.uniform(0, 24, size=n), [0.0]]))
        objs.append(np.concatenate([cls, [0]]))
        rows.append(n + 1)
    T = torch.from_numpy
    return dict(S=S, R=R, V=V, near=near, boxes=T(np.concatenate(boxes).astype(np.float32)), angles=T(np.concatenate(angles).astype(np.float32)),
                objs=T(np.concatenate(objs).astype(np.int64)), rows=rows, draws=T(rng.random((R, V, 2)).astype(np.float32)))


def torch_route(SH, bnk, c, dtype, rasterize=None):
    """faces_xyz / face_label of ``place_project_torch`` in ``dtype`` on the host (and the whole of ``views_torch`` with a rasterizer)"""
    if rasterize is not None:
        return SH.views_torch(bnk, c["boxes"], c["angles"], c["objs"], c["rows"], c["draws"], rasterize, size=c["S"], views=c["V"], near=c["near"],
                              dtype=dtype)
    tables = SH.BankTables.of(bnk, "cpu")
    bind = SH.Binding(c["rows"], None, "cpu")
    choice = pkg("host.retrieve").retrieve_models_torch(c["boxes"], c["objs"], bind.room_row, bnk.table)
    rt = SH.row_tables(tables, bind, c["boxes"], c["angles"], c["objs"], choice, dtype)
    shell_v = SH.procedural_shell(tables, rt["ext"].float())
    d = c["draws"].to(dtype)
    K, Rm, t = SH.shade_camera(rt["ext"][:, None, :].expand(c["R"], c["V"], 3), d[..., 0], d[..., 1], c["S"])
    fxyz, flabel = SH.place_project_torch(tables, rt, shell_v, K, Rm, t, c["S"], c["near"])
    return dict(faces_xyz=fxyz, face_label=flabel, rt=rt)


def face_error(got, want):
    """largest |got - want| / max(1, |want|) over the faces that both keep, and the number of faces only one of them culled"""
    got, want = got.double(), want.double()
    dead_g, dead_w = (got == 0).all(-1).all(-1), (want == 0).all(-1).all(-1)
    both = ~dead_g & ~dead_w
    err = ((got - want).abs() / want.abs().clamp(min=1.0))[both]
    return (float(err.max()) if err.numel() else 0.0), int((dead_g != dead_w).sum())


def shell_bank(device):
    """``bank`` with shell meshes (two wall sub-meshes over one vertex list, a floor, a ceiling): its shell is placed on the host"""
    RF = pkg("host.refine")
    wv, wf = _cuboid((4.0, 2.5, 5.0), 2, shift=(2.0, 1.25, 2.5))
    fv, ff = _cuboid((4.0, 0.1, 5.0), 1, shift=(2.0, -0.05, 2.5))
    cv, cf = _cuboid((4.0, 0.1, 5.0), 1, shift=(2.0, 0.05, 2.5))
    back, left = wf[:8], wf[16:24]                                       # two of the cuboid's faces as the wall's sub-meshes
    shell = dict(wall_v=wv, wall_f=[back, left], wall_bbox=[[0, 0, 0], [4.0, 2.5, 5.0]], floor_v=fv, floor_f=ff, floor_bbox=[[0, -0.1, 0], [4.0, 0.0, 5.0]],
                 ceil_v=cv, ceil_f=cf)
    meshes = {"bed": _cuboid((2.0, 0.5, 1.5), 1), "desk": _cuboid((1.4, 0.75, 0.7), 2)}
    return RF.MeshBank.from_arrays(meshes, device, vocab=VOCAB[1:], shell=shell)
