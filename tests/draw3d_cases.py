"""Cases shared by tests/test_draw3d_host.py and tests/test_draw3d_gpu.py (host/draw3d.py, csrc/draw3d.hip): the rooms of
shade_view_cases at the sample counts per pixel they are drawn with, hand-made operand cases that need no renderer, and the comparison
the operand tests use."""
import functools

import numpy as np
import torch

import shade_view_cases as CS
from conftest import pkg

FAR = 100.0
CHUNK = 256                         # faces per pass of csrc/draw3d.hip's lighting kernel
UNSAFE_CAP = 0.005                  # share of the hit samples that may be unsafe, per case
# room case of shade_view_cases -> the k (samples per output pixel and axis) it is drawn with: k = 3 gives 15 x 15 tiles, k = 4 16 x 16
ROOMS = {"one_view": (1, 4), "five_views": (1, 3), "five_views_100": (1, 4), "seventeen_rooms": (4,), "seventeen_views": (1,), "no_visible_row": (1,),
         "every_face_culled": (1,)}
HAND = ("floor", "occluder", "soup_200", "soup_255", "soup_256", "soup_257", "soup_600", "index_outside", "label_above_40", "lamp_behind",
        "chosen_by_hand")


def room_ext(c):
    last = torch.tensor(np.cumsum(c["rows"]) - 1)
    return (c["boxes"][last, 3:] - c["boxes"][last, :3]).double()


def room_operands(name, dtype=torch.float64):
    """The operands of ``draw3d_torch`` for a room case, from ``views_torch`` in ``dtype`` with the rasterizer's C restatement -> dict
    (faces_xyz float32 - what the rasterizer saw -, face_index, depth in raster order, face_label, chosen, K, light_cam float64, S, ks)"""
    from oracle import raster_ref
    SH, D = pkg("host.shade"), pkg("host.draw3d")
    c = CS.case(name)
    out = CS.torch_route(SH, CS.bank("cpu"), c, dtype, raster_ref.nmr_forward)
    R, V = c["R"], c["V"]
    pick = torch.arange(R) * V + out["chosen"]
    light_cam = D.light_in_camera(D.light_position(room_ext(c)), out["R"].reshape(R * V, 3, 3)[pick].double(), out["t"].reshape(R * V, 3)[pick].double())
    return dict(faces_xyz=out["faces_xyz"].float(), face_index=out["face_index"], depth=torch.flip(out["depth_all"], [1]).contiguous(),
                face_label=out["face_label"], chosen=out["chosen"], K=out["K"].reshape(R * V, 3, 3).float(), light_cam=light_cam, S=c["S"],
                ks=ROOMS[name], background=(0.0, 0.0, 0.0), status=out["status"])


# ------------------------------------------------------------------------------------------------------------------------------
# hand-made operands: faces given in the camera frame (x right, y down, z forwards), K of the module's convention
# ------------------------------------------------------------------------------------------------------------------------------
def _quad(cx, cy, z, half):
    """two triangles of the square |x - cx|, |y - cy| <= half in the plane z"""
    a, b, c, d = (cx - half, cy - half, z), (cx + half, cy - half, z), (cx + half, cy + half, z), (cx - half, cy + half, z)
    return [[a, b, c], [a, c, d]]


def _to_ndc(tris):
    """camera-frame triangles [F, 3, 3] -> (x_ndc, y_ndc, z_cam) float32 with the winding the rasterizer keeps"""
    t = np.asarray(tris, np.float64)
    z = np.where(t[..., 2] == 0, 1.0, t[..., 2])                    # (a triangle at the origin is a collapsed slot: it stays there)
    out = np.stack((2.0 * t[..., 0] / z, -2.0 * t[..., 1] / z, t[..., 2]), -1)
    cross = (out[:, 1, 0] - out[:, 0, 0]) * (out[:, 2, 1] - out[:, 0, 1]) - (out[:, 2, 0] - out[:, 0, 0]) * (out[:, 1, 1] - out[:, 0, 1])
    back = cross < 0
    out[back] = out[back][:, [0, 2, 1]]
    return out.astype(np.float32)


FLOOR_Z, LAMP = 3.0, (0.2, -0.1, 1.5)
OCCLUDER = (0.2, -0.1, 2.25, 0.2)                   # centre x, y, depth, half side: its umbra on the floor is the square of half side 0.4


def _soup(F, S, rng):
    """F faces: the floor (2, last), four slivers laid across the corner samples' segments of two tiles - 1 % of the way to the lamp, just
    inside the tile's segment bundle, and as far beyond the corner, just outside it -, the rest small triangles between lamp and floor
    (equilateral, in random planes: a needle's normal would amplify the float32 rounding of its corners beyond what the rooms' faces show)"""
    tris = []
    for _ in range(F - 6):
        ctr = rng.uniform([-1.2, -1.2, 1.8], [1.2, 1.2, 2.9])
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.0, 4.0]) * np.pi / 3
        tris.append(ctr + rng.uniform(0.06, 0.25) * (np.cos(ang)[:, None] * q[0] + np.sin(ang)[:, None] * q[1]))
    lamp = np.asarray(LAMP)
    for yi, xi in ((0, 0), (S // 2, S // 2)):
        corner = np.array([(2 * xi + 1 - S) / S / 2.0, -(2 * yi + 1 - S) / S / 2.0, 1.0]) * FLOOR_Z
        way = (lamp - corner) / np.linalg.norm(lamp - corner)
        side = np.cross(way, [0.0, 0.0, 1.0]); side /= np.linalg.norm(side)
        up = np.cross(way, side)
        for along in (0.03, -0.03):                  # inside the bundle (across the segment) and outside it (behind the corner)
            at = corner + along * way
            tris.append(np.stack((at - 0.05 * side - 0.03 * up, at + 0.05 * side - 0.03 * up, at + 0.06 * up)))
    tris = [np.asarray(t) for t in tris] + [np.asarray(t, np.float64) for t in _quad(0.0, 0.0, FLOOR_Z, 2.0)]
    return np.stack(tris)


def hand(name):
    """-> the operand dict of ``room_operands`` for a hand-made case (float32 / int32 / uint8 / int64 tensors on the host)"""
    from oracle import raster_ref
    S, R, V, ks, bg, lamp, chosen = 32, 1, 1, (1, 4), (0.0, 0.0, 0.0), LAMP, [0]
    floor = _quad(0.0, 0.0, FLOOR_Z, 1.0)
    occ = _quad(*OCCLUDER)
    if name == "floor":
        views, labels, bg = [floor], [[2, 2]], (0.25, 0.5, 0.125)
    elif name in ("occluder", "index_outside", "label_above_40", "lamp_behind"):
        views, labels = [floor + occ], [[2, 2, 5, 5]]
        if name == "label_above_40":
            labels = [[2, 200, 41, 40]]
        if name == "lamp_behind":
            lamp = (0.2, -0.1, 5.0)
    elif name.startswith("soup_"):
        F = int(name[5:])
        S, ks = 48, (1, 3)
        rng = np.random.default_rng(F)
        views, labels = [_soup(F, S, rng)], [list(rng.integers(1, 41, size=F - 2)) + [2, 2]]
    elif name == "chosen_by_hand":
        R, V, chosen = 2, 3, [2, 1]
        pad = [[(0.0, 0.0, 0.0)] * 3] * 2
        far_floor = _quad(0.3, 0.2, 4.0, 1.5)
        views = [far_floor + pad, pad + pad, floor + occ, occ + pad, far_floor + occ, pad + floor]
        labels = [[2, 2, 5, 5], [3, 3, 7, 7]]
    else:
        raise KeyError(name)
    faces = np.stack([_to_ndc(v) for v in views])
    fi, _, dep = raster_ref.nmr_forward(faces, S, 0.1, FAR)
    fi, dep = np.ascontiguousarray(fi), np.ascontiguousarray(dep)
    F = faces.shape[1]
    if name == "index_outside":
        fi[0, 3, :] = -1; fi[0, 5, ::2] = F; fi[0, 7, 1::3] = F + 1000; fi[0, S // 2, S // 2] = F
    K = torch.tensor([[S, 0, S / 2], [0, S, S / 2], [0, 0, 1]], dtype=torch.float32).expand(R * V, 3, 3).contiguous()
    return dict(faces_xyz=torch.from_numpy(faces), face_index=torch.from_numpy(fi), depth=torch.from_numpy(dep),
                face_label=torch.tensor(labels, dtype=torch.uint8), chosen=torch.tensor(chosen, dtype=torch.int64), K=K,
                light_cam=torch.tensor([lamp] * R, dtype=torch.float32).double(), S=S, ks=ks, background=bg)


def reference(op, k, dtype=torch.float64, **kw):
    D = pkg("host.draw3d")
    return D.draw3d_torch(op["faces_xyz"], op["face_index"], op["depth"], op["face_label"], op["chosen"], op["K"], op["light_cam"], k,
                          background=op["background"], dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def operands(name):
    """the operand dict of a room or hand-made case, built once and shared: treat it as read-only"""
    return room_operands(name) if name in ROOMS else hand(name)


@functools.lru_cache(maxsize=None)
def want(name):
    """``draw3d_torch`` in float64 on ``operands(name)`` at the case's first k (``linear``, ``hit``, ``visible`` and ``unsafe`` do not
    depend on k), computed once and shared: treat it as read-only"""
    op = operands(name)
    return reference(op, op["ks"][0])


def linear_error(got, want):
    """largest |got - want| / max(1, |want|) over the hit samples that are safe in ``want`` (a ``draw3d_torch`` result), the share of
    the hit samples that are unsafe, and the number of hit samples"""
    safe = want["hit"] & ~want["unsafe"]
    lin = want["linear"].double()
    err = ((got.double() - lin).abs() / lin.abs().clamp(min=1.0))[safe]
    hits = int(want["hit"].sum())
    return (float(err.max()) if err.numel() else 0.0), (float((want["hit"] & want["unsafe"]).sum()) / hits if hits else 0.0), hits
