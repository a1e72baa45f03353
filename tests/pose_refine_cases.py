"""The operands of the pose-gradient tests (sln_place_pose_step_views), on the CPU for tests/test_pose_refine_host.py and on the GPU for
tests/test_place_pose_gpu.py: two rooms of tests/test_place_views_gpu.py's kind -

  * room 0: the 7 rows of tests/test_refine_gpu.py over the procedural bank - 5 visible cuboids of 48 faces and a shell of 360: 600 faces,
    a lane of the 256 walks two or three of them;
  * room 1: 5 rows over a coarse bank - 4 cuboids of 12 faces and a shell of 10 (three walls, floor, ceiling of two triangles each): 58
    faces, three of the four wavefronts idle

- their cameras (``cameras("three")``: the refinement camera, one from outside that culls nothing, one from inside object 0 that culls part;
``cameras("away")``: one that culls every face, then the outside one) and random face gradients."""
import functools

import numpy as np
import torch

from conftest import pkg

import test_refine_gpu as TR

NAMES_B = ["cabinet", "lamp", "sofa", "television", "__room__"]
EXT_B = (3.6, 2.5, 4.4)
IMAGE = 64


def _boxes_b(dev):
    g = torch.Generator().manual_seed(7)
    n = len(NAMES_B)
    lo = torch.rand(n, 3, generator=g) * 0.45 + 0.05
    lo[:, 1] = 0.0; lo[:, 2] = lo[:, 2] * 0.6
    boxes = torch.cat([lo, lo + torch.rand(n, 3, generator=g) * 0.2 + 0.12], 1)
    boxes[-1] = torch.tensor([0, 0, 0, *EXT_B])
    return boxes.to(dev), torch.randint(0, 24, (n,), generator=g).float().to(dev)


def _coarse_bank(dev):
    """12-face cuboids and a shell of two triangles per surface, in room 1's own extent (the shell tables scale it by exactly 1)"""
    R, syn = pkg("host.refine"), pkg("host.synthetic")
    rng = np.random.default_rng(11)
    meshes = {}
    for name in NAMES_B[:-1]:
        size = rng.uniform(0.5, 1.5, size=3)
        meshes[name] = syn._grid_cuboid(-size / 2, size / 2, 1)
        assert meshes[name][1].shape[0] == 12
    ex, ey, ez = EXT_B
    box = np.array([[0, 0, 0], [ex, 0, 0], [0, ey, 0], [ex, ey, 0], [0, 0, ez], [ex, 0, ez], [0, ey, ez], [ex, ey, ez]], dtype=np.float32)
    quad = lambda a, b, c, d: np.array([[a, b, c], [c, b, d]])
    shell = dict(wall_v=box, wall_f=[quad(0, 1, 2, 3), quad(0, 2, 4, 6), quad(1, 5, 3, 7)], wall_bbox=np.array([[0, 0, 0], EXT_B]),
                 floor_v=box[[0, 1, 4, 5]], floor_f=quad(0, 1, 2, 3), floor_bbox=np.array([[0, 0, 0], [ex, 0, ez]]),
                 ceil_v=box[[2, 3, 6, 7]], ceil_f=quad(0, 1, 2, 3))
    return R.MeshBank.from_arrays(meshes, dev, shell=shell)


@functools.lru_cache(maxsize=None)
def rooms(dev):
    """[(class names, boxes [n, 6], angle bins [n] (fractional), scene, size targets [n_vis, 3])] of the two rooms on ``dev``"""
    R = pkg("host.refine")
    banks = (R.MeshBank(TR.FURN, dev, seed=3), _coarse_bank(dev))
    out = []
    for bank, names, (boxes, angles) in zip(banks, (TR.NAMES, NAMES_B), (TR._inputs(dev), _boxes_b(dev))):
        scene = R.RefineScene(names, bank, boxes[-1].clone(), image_size=IMAGE)
        tgt = torch.stack([torch.tensor([0.5, 0.4, 0.6]) * (1 + 0.1 * k) for k in range(scene.n_vis)]).to(dev).contiguous()
        out.append((names, boxes.contiguous(), (angles + 0.3).contiguous(), scene, tgt))
    assert [int(rm[1].shape[0]) for rm in out] == [7, 5]
    assert out[0][3].desc.F > 256 and out[1][3].desc.F < 64, [rm[3].desc.F for rm in out]
    return out


def _object_centre(room, k=0):
    _, boxes, _, scene, _ = room
    b, ext = boxes[int(scene.vis[k])].cpu().double(), boxes[-1, 3:].cpu().double()
    return ((b[:3] + b[3:]) / 2 * ext).numpy()


@functools.lru_cache(maxsize=None)
def cameras(which, dev):
    """per room a list of (K [3, 3], R [3, 3], t [3]) float32 on the host (tests/test_place_views_gpu.py::_cameras)"""
    RP = pkg("host.reproject")
    cams = []
    for room in rooms(dev):
        ext = room[1][-1, 3:].cpu().double().numpy()
        own = RP.refine_view(room[1][-1], IMAGE)[:3]
        outside = RP.look_at_view(ext + [1.5, 1.0, 2.0], ext / 2)[:3]
        c = _object_centre(room)
        close = RP.look_at_view(c, c + [-1.0, -0.2, -1.0])[:3]
        front = np.array([ext[0] / 2, ext[1] / 2, ext[2] + 1.0])
        away = RP.look_at_view(front, front + [0.0, 0.0, 1.0])[:3]
        cams.append(dict(three=[own, outside, close], away=[away, outside])[which])
    return cams


def face_counts(dev):
    return [rm[3].desc.F for rm in rooms(dev)]


def grad_faces(V, dev, seed=1):
    """[R * V, F2, 3, 3] float32 with F2 = 2 max F: the same numbers on every device"""
    F2 = 2 * max(face_counts(dev))
    return torch.randn(2 * V, F2, 3, 3, generator=torch.Generator().manual_seed(seed)).to(dev)


def host_operands(which, dev="cpu"):
    """per (room, view): dict(r, v, faces [F, 3], corners [Vtot, 3] float32 from ``RefineScene.place`` on ``dev``, K, R, t, grad_faces [2F, 3, 3],
    orig_size, proj_eps, cull_eps) as numpy - what ``pose_refine_ref.pose_grad_ref`` takes"""
    cams = cameras(which, dev)
    V = len(cams[0])
    gf = grad_faces(V, dev).cpu().numpy()
    out = []
    for r, (names, boxes, angles, scene, _) in enumerate(rooms(dev)):
        with torch.no_grad():
            corners = scene.place(boxes, angles)[0][0].float().cpu().numpy()
        d = scene.desc
        for v, (K, Rm, t) in enumerate(cams[r]):
            out.append(dict(r=r, v=v, faces=scene.faces.cpu().numpy(), corners=corners, K=K.numpy(), R=Rm.numpy(), t=t.numpy(),
                            grad_faces=gf[r * V + v, :2 * d.F], orig_size=d.orig_size, proj_eps=d.proj_eps, cull_eps=d.cull_eps))
    return out
