"""Draw a layout in 3-D on the device: the ``--draw_3d`` path of the reference's ``test.py`` (testing/test_plot3d.py::run_blender ->
render/render_caller.py -> render/render_room_color.py::render_test), which starts Blender once per layout.  As far as geometry goes
that ``render_test`` is render_semantic_depth.py's statement for statement (tests/golden/draw3d.npz records that their syntax trees are
equal), so everything up to "which face does every pixel of the accepted view see, and how far away" is ``shade.ViewRenderer``.  From
there to colour:

  * ``draw3d_torch``    the shading model below in torch ops on any device, float64 or float32: the yardstick and the CPU route;
  * ``Draw3D``          static buffers around a ``ViewRenderer`` and the two launches of ``sln_draw3d`` (csrc/draw3d.hip);
  * ``render_test_3d``  render_caller.py:22-42 for a ``data_extracted.json``-shaped dict: four predictions per room, the reference's
    file names.

The shading model is OURS, not Blender's (Cycles' 50-sample path tracing, the HDR environment, textures and soft shadows are out of
reach): per raster sample of the accepted view, in that view's camera frame, background where ``face_index`` is outside [0, F); else
``albedo[label] * (ambient + intensity * vis * c / d^2)`` with the hit point ``p = ray(pixel centre) * depth``, the face's normal turned
towards the camera (faces are two-sided), ``l = light - p``, ``d^2 = max(|l|^2, min_dist^2)``, ``c = max(0, n.l / |l|)`` and ``vis = 0``
when the segment from ``p + bias n`` to the lamp meets another face (two-sided Moller-Trumbore; ``t`` in (0, 1), barycentrics in [0, 1]; a
zero determinant - every collapsed slot - is no hit).  The picture is the k x k box filter of the linear samples, sRGB-encoded.  What the
reference's source does state is kept: the lamp at (X / 2, 0.9 Y, Z / 2) with size 0.1 (:405-406), 1024 pixels at 25 % (:348-350), the
file names.
"""
import os

import torch

from .. import _lib as L
from . import shade as SH
from .scene_pictures import CLASS_COLORS, _folder, _write

LIGHT_AT = (0.5, 0.9, 0.5)          # :405 as fractions of the room's extent
LIGHT_ENERGY = 1.2                  # :406 (Blender's unit; the model's ``intensity`` is its own parameter)
LIGHT_SIZE = 0.1                    # :406: the lamp's size, the model's smallest distance
RESOLUTION = 1024                   # :348-349
RESOLUTION_PERCENTAGE = 25          # :350
N_PRED = 4                          # render_caller.py:38
AMBIENT, INTENSITY, BIAS, DELTA = 0.35, 3.0, 1e-3, 1e-4
_TINY = 1e-30


def light_position(room_ext):
    """:405: the lamp of a room of extent ``room_ext`` [..., 3] (a tensor or a sequence of floats) in the room's frame"""
    e = room_ext if torch.is_tensor(room_ext) else torch.as_tensor(room_ext, dtype=torch.float64)      # (host floats are doubles)
    e = e if e.is_floating_point() else e.double()
    return torch.stack((e[..., 0] / 2, e[..., 1] * 0.9, e[..., 2] / 2), -1)


def srgb_to_linear(c):
    """the sRGB transfer function's inverse on values in [0, 1]"""
    return torch.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def linear_to_srgb(c):
    c = c.clamp(0.0, 1.0)
    return torch.where(c <= 0.0031308, 12.92 * c, 1.055 * c.clamp(min=_TINY) ** (1.0 / 2.4) - 0.055)


def albedo_table(device=None):
    """[41, 3] float32: ``scene_pictures.CLASS_COLORS`` from sRGB bytes to linear colour, computed in float64; entry 0 is black"""
    c = torch.tensor(CLASS_COLORS, dtype=torch.float64) / 255.0
    return srgb_to_linear(c).float().to(device)


def percentage_k(size, percentage):
    """samples per output pixel and axis: ``P = size * percentage / 100`` and ``k = size / P`` must be integers, k in [1, 16]"""
    P = int(size) * percentage / 100.0
    if P < 1 or P != int(P) or int(size) % int(P) != 0 or not 1 <= int(size) // int(P) <= 16:
        raise ValueError("size %r at %r %%: the picture's side and size / side must be integers, the latter in [1, 16]" % (size, percentage))
    return int(size) // int(P)


def encode_picture(linear, k):
    """``linear`` [R, S, S, 3] in raster order -> uint8 [R, S / k, S / k, 3] in image row order: the mean of every k x k block (added row
    by row), clamped to [0, 1], sRGB-encoded, times 255, rounded to nearest"""
    R, S = linear.shape[0], linear.shape[1]
    P = S // k
    blk = linear.reshape(R, P, k, P, k, 3)
    acc = torch.zeros(R, P, P, 3, dtype=linear.dtype, device=linear.device)
    for j in range(k):
        for i in range(k):
            acc = acc + blk[:, :, j, :, i]
    byte = torch.floor(linear_to_srgb(acc / float(k * k)) * 255.0 + 0.5)
    return torch.flip(byte.to(torch.uint8), [1]).contiguous()


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return torch.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def camera_faces(faces_xyz, K, S):
    """(x_ndc, y_ndc, z_cam) [..., F, 3, 3] back to the camera frame with ``fx, fy, cx, cy`` of ``K`` [..., 3, 3] (no skew,
    ``orig_size = S``) -> (corners [..., F, 3, 3], (ax, bx, ay, by) with x / z = x_ndc * ax + bx and y / z = y_ndc * ay + by)"""
    S = float(S)
    fx, cx, fy, cy = K[..., 0, 0], K[..., 0, 2], K[..., 1, 1], K[..., 1, 2]
    ax, bx, ay, by = S / (2.0 * fx), (S / 2.0 - cx) / fx, -S / (2.0 * fy), (S / 2.0 - cy) / fy
    z = faces_xyz[..., 2]
    e = lambda v: v[..., None, None]
    pts = torch.stack(((faces_xyz[..., 0] * e(ax) + e(bx)) * z, (faces_xyz[..., 1] * e(ay) + e(by)) * z, z), -1)
    return pts, (ax, bx, ay, by)


def _shadow_tests(o, d, own, v0, e1, e2, face_id, delta, budget=1 << 21):
    """segments ``o + t d`` [n, 3] against faces (v0, e1, e2) [m, 3] -> three bool [n]: hit by the test as stated, with the bounds widened by
    ``delta`` and with them narrowed by ``delta``.  ``own`` [n] is the face a segment starts on (skipped)."""
    n, m = o.shape[0], v0.shape[0]
    out = [torch.zeros(n, dtype=torch.bool, device=o.device) for _ in range(3)]
    step = max(1, budget // max(n, 1))
    o, d = o[:, None, :], d[:, None, :]
    for a in range(0, m, step):
        w0, w1, w2 = v0[None, a:a + step], e1[None, a:a + step], e2[None, a:a + step]
        pv = _cross(d, w2)
        det = _dot(w1, pv)
        ok = (det != 0) & (face_id[None, a:a + step] != own[:, None])
        inv = 1.0 / torch.where(det != 0, det, torch.ones_like(det))
        tv = o - w0
        u = _dot(tv, pv) * inv
        qv = _cross(tv, w1)
        v = _dot(d, qv) * inv
        t = _dot(w2, qv) * inv
        for slot, s in enumerate((0.0, delta, -delta)):          # as stated, widened, narrowed
            h = ok & (u >= -s) & (v >= -s) & (u + v <= 1.0 + s) & (t > -s) & (t < 1.0 + s)
            out[slot] |= h.any(dim=1)
    return out


def draw3d_torch(faces_xyz, face_index, depth, face_label, chosen, K, light_cam, k, albedo=None, ambient=AMBIENT, intensity=INTENSITY,
                 min_dist=LIGHT_SIZE, bias=BIAS, background=(0.0, 0.0, 0.0), shadows=True, dtype=torch.float64, delta=DELTA):
    """The shading model in torch ops on the operands' device, in ``dtype``.  ``faces_xyz`` [R * V, F, 3, 3], ``face_index`` / ``depth``
    [R * V, S, S] in raster order, ``face_label`` [R, F] uint8, ``chosen`` [R], ``K`` [R * V, 3, 3] (or [R, V, 3, 3]), ``light_cam`` [R, 3].
    -> dict(linear [R, S, S, 3] ``dtype`` in raster order, picture uint8 [R, S / k, S / k, 3] in image row order, visible [R, S, S] (no
    face between the sample and the lamp, or no ray cast), hit [R, S, S], unsafe [R, S, S]: the shadow decision changes between the test
    with its bounds widened by ``delta`` and with them narrowed, or the view ray grazes the face (|n.p| / (|n| |p|) < ``delta``))."""
    dev = faces_xyz.device
    R, F = face_label.shape
    B, S = face_index.shape[0], face_index.shape[1]
    V = B // R
    b = torch.arange(R, device=dev) * V + chosen.long().clamp(0, V - 1)
    pts, (ax, bx, ay, by) = camera_faces(faces_xyz[b].to(dtype), K.reshape(B, 3, 3)[b].to(dtype), S)
    v0, e1, e2 = pts[:, :, 0], pts[:, :, 1] - pts[:, :, 0], pts[:, :, 2] - pts[:, :, 0]
    fi = face_index[b].long()
    hit = (fi >= 0) & (fi < F)
    fc = torch.where(hit, fi, torch.zeros_like(fi))
    z = depth[b].to(dtype)
    ar = torch.arange(S, device=dev)
    pc = (2 * ar + 1 - S).to(dtype) / float(S)
    e = lambda v: v[:, None, None]
    p = torch.stack(((pc[None, None, :] * e(ax) + e(bx)) * z, (pc[None, :, None] * e(ay) + e(by)) * z, z), -1)
    room = torch.arange(R, device=dev)[:, None, None]
    n = _cross(e1[room, fc], e2[room, fc])
    n = n / torch.sqrt(_dot(n, n).clamp(min=_TINY))[..., None]
    facing = _dot(n, p)
    n = torch.where((facing > 0)[..., None], -n, n)
    light = light_cam.to(dtype)[:, None, None, :]
    l = light - p
    ll = _dot(l, l)
    d2 = ll.clamp(min=float(min_dist) ** 2)
    c = (_dot(n, l) / torch.sqrt(ll.clamp(min=_TINY))).clamp(min=0.0)
    unsafe = hit & (facing.abs() / torch.sqrt(_dot(p, p).clamp(min=_TINY)) < delta)
    need = hit & (c > 0) & bool(shadows)
    shadowed = torch.zeros_like(hit)
    org = p + float(bias) * n
    for r in range(R):
        at = need[r].nonzero(as_tuple=True)
        if at[0].numel() == 0:
            continue
        live = ((e1[r] != 0) | (e2[r] != 0)).any(-1).nonzero().flatten()       # (a collapsed slot has a zero determinant for every ray)
        o = org[r][at]
        h, wide, narrow = _shadow_tests(o, light[r, 0, 0] - o, fi[r][at], v0[r, live], e1[r, live], e2[r, live], live, delta)
        shadowed[r][at] = h
        unsafe[r][at] |= wide != narrow
    vis = ~shadowed
    E = float(ambient) + float(intensity) * torch.where(vis, c, torch.zeros_like(c)) / d2
    lab = face_label[room, fc].long()
    alb = (albedo_table(dev) if albedo is None else albedo).to(dtype)[torch.where(lab <= 40, lab, torch.zeros_like(lab))]
    bg = torch.tensor([float(x) for x in background], dtype=dtype, device=dev)
    linear = torch.where(hit[..., None], alb * E[..., None], bg.expand(R, S, S, 3))
    return dict(linear=linear, picture=encode_picture(linear, int(k)), visible=vis, hit=hit, unsafe=unsafe)


def light_in_camera(light, Rm, t):
    """``Rm`` [n, 3, 3] . ``light`` [n, 3] + ``t`` [n, 3] as a written-out sum"""
    return ((Rm[:, :, 0] * light[:, None, 0] + Rm[:, :, 1] * light[:, None, 1]) + Rm[:, :, 2] * light[:, None, 2]) + t


# ------------------------------------------------------------------------------------------------------------------------------
# the device route
# ------------------------------------------------------------------------------------------------------------------------------
def draw3d_launch(faces_xyz, face_index, depth, face_label, chosen, K, light_cam, albedo, k, workspace, picture, linear=None, ambient=AMBIENT,
                  intensity=INTENSITY, min_dist=LIGHT_SIZE, bias=BIAS, background=(0.0, 0.0, 0.0), shadows=True):
    """the bare ``sln_draw3d`` call (two launches) over the caller's contiguous buffers"""
    d = L.SlnDraw3D()
    P = lambda x: x.data_ptr()
    d.faces_xyz, d.face_index, d.depth, d.face_label, d.chosen = P(faces_xyz), P(face_index), P(depth), P(face_label), P(chosen)
    d.K, d.light_cam, d.albedo = P(K), P(light_cam), P(albedo)
    d.R, d.F = int(face_label.shape[0]), int(face_label.shape[1])
    d.V, d.S, d.k, d.shadows = int(face_index.shape[0]) // max(d.R, 1), int(face_index.shape[1]), int(k), int(bool(shadows))
    d.ambient, d.intensity, d.min_dist, d.bias = float(ambient), float(intensity), float(min_dist), float(bias)
    d.background[0], d.background[1], d.background[2] = (float(x) for x in background)
    L.check(L.lib().sln_draw3d(d, L.ptr(workspace), L.ptr(picture), L.ptr(linear), SH._stream(picture)), "sln_draw3d")


class Draw3D:
    """The lit colour picture of the rooms of a ``ViewRenderer`` on the device.

        renderer = ViewRenderer(bank, size=1024, views=5, batch=R)
        draw = Draw3D(renderer)
        picture, status = draw.draw3d(boxes, angles, objs, rows)          # render, then light
        picture, status = draw.draw3d()                                   # light again what the last call left

    ``picture`` uint8 [R, P, P, 3] with ``P = size * percentage / 100``, image row order; ``status`` is the renderer's: a room without an
    accepted view is drawn from view 0 and flagged.  ``linear=True`` also keeps the linear samples (``self.linear`` [R, S, S, 3], raster
    order).  The results are static buffers; nothing is read back, ``chosen`` is read on the device, so a captured call replays with
    another choice.  The buffers that follow the rooms' lengths are built on the first call with arguments (not inside a capture)."""

    def __init__(self, renderer, percentage=RESOLUTION_PERCENTAGE, ambient=AMBIENT, intensity=INTENSITY, background=(0, 0, 0), shadows=True,
                 linear=False):
        self.device = torch.device(getattr(renderer, "device", "cpu"))
        if self.device.type != "cuda":
            raise L.SlnError("Draw3D runs on the MI355X only (no CPU fallback); draw3d_torch restates it for host tensors")
        self.renderer, self.k = renderer, percentage_k(renderer.size, percentage)
        self.ambient, self.intensity, self.background, self.shadows = float(ambient), float(intensity), tuple(float(x) for x in background), bool(shadows)
        if len(self.background) != 3:
            raise ValueError("background: three linear colour values expected")
        R, V, S, dev = renderer.batch, renderer.views, renderer.size, self.device
        self.P = S // self.k
        self.picture = torch.zeros(R, self.P, self.P, 3, dtype=torch.uint8, device=dev)
        self.linear = torch.zeros(R, S, S, 3, dtype=torch.float32, device=dev) if linear else None
        self.albedo = albedo_table(dev).contiguous()
        self.K = torch.zeros(R * V, 3, 3, dtype=torch.float32, device=dev)
        self._Rm = torch.zeros(R * V, 3, 3, dtype=torch.float32, device=dev)
        self._t = torch.zeros(R * V, 3, dtype=torch.float32, device=dev)
        self._light = torch.zeros(R, 3, dtype=torch.float32, device=dev)
        self.light_cam = torch.zeros(R, 3, dtype=torch.float32, device=dev)
        self._ws, self._ws_F, self._ready = None, -1, False

    def _workspace(self):
        r = self.renderer
        if self._ws_F != r.F:
            n = int(L.lib().sln_draw3d_workspace_bytes(r.batch, r.F))
            if n < 0:
                L.check(n, "sln_draw3d_workspace_bytes")
            self._ws, self._ws_F = torch.empty(n // 4, dtype=torch.float32, device=self.device), r.F
        return self._ws

    def draw3d(self, boxes=None, angles=None, objs=None, rows=None, draws=None, generator=None):
        r = self.renderer
        if boxes is not None:
            if draws is None:
                draws = torch.rand(r.batch, r.views, 2, device=self.device, generator=generator)
            r(boxes, angles, objs, rows, draws=draws)
            # the cameras the renderer formed, by its own statements on its own inputs
            room = boxes[r._bind.last]
            ext = room[:, 3:] - room[:, :3]
            d = draws.to(device=self.device, dtype=torch.float32)
            K, Rm, t = SH.shade_camera(ext[:, None, :].expand(r.batch, r.views, 3), d[..., 0], d[..., 1], r.size)
            self.K.copy_(K.reshape(-1, 3, 3)); self._Rm.copy_(Rm.reshape(-1, 3, 3)); self._t.copy_(t.reshape(-1, 3))
            self._light.copy_(light_position(ext))
            self._ready = True
        elif not self._ready:
            raise ValueError("draw3d() lights what the last draw3d(boxes, angles, objs, rows) left: there was none")
        pick = r._room0 + r.chosen
        self.light_cam.copy_(light_in_camera(self._light, self._Rm[pick], self._t[pick]))
        draw3d_launch(r.faces_xyz, r.face_index, r._raster_depth, r.face_label, r.chosen, self.K, self.light_cam, self.albedo, self.k,
                      self._workspace(), self.picture, self.linear, ambient=self.ambient, intensity=self.intensity, background=self.background,
                      shadows=self.shadows)
        return self.picture, r.status

    __call__ = draw3d


def picture_names(data):
    """render_caller.py:28-42: the file names of a ``data_extracted.json``-shaped dict, in the order they are written"""
    return [room_id + "_pred_" + str(k).zfill(2) + "_3d.png" for room_id in data for k in range(N_PRED)]


def render_test_3d(data, bank, out_dir, vocab=None, size=RESOLUTION, rng=None):
    """render_caller.py::render_test_3d (:22-42) for ``data`` = {room_id: {"gt": {"objs": [...]}, "0": {"boxes": [...], "angles": [...]},
    ... "3": {...}}} (the content of ``data_extracted.json``; boxes room-normalised with the room row last, as ``render_test`` takes
    them): the four predictions of every room are rendered and lit in one call and written as ``<room_id>_pred_<0k>_3d.png`` into
    ``out_dir``.  Rooms of equal length share a bound renderer.  ``rng``: the torch generator of the viewpoint draws.  Files need PIL (a
    warning otherwise).  -> the written paths."""
    _folder(out_dir)
    dev = next(iter(bank.models.values()))["v"].device if bank.models else torch.device("cuda")
    drawers, paths = {}, []
    for room_id, room_data in data.items():
        objs = [int(o) for o in room_data["gt"]["objs"]]
        n = len(objs)
        if n not in drawers:
            drawers[n] = Draw3D(SH.ViewRenderer(bank, size=size, views=SH.N_SAMPLE, batch=N_PRED, vocab=vocab, device=dev))
        boxes = torch.tensor([row for k in range(N_PRED) for row in room_data[str(k)]["boxes"]], dtype=torch.float32, device=dev)
        angles = torch.tensor([a for k in range(N_PRED) for a in room_data[str(k)]["angles"]], dtype=torch.float32, device=dev)
        picture, _ = drawers[n].draw3d(boxes, angles, torch.tensor(objs * N_PRED, dtype=torch.int64, device=dev), [n] * N_PRED, generator=rng)
        for k in range(N_PRED):
            path = _write(picture[k], os.path.join(out_dir, room_id + "_pred_" + str(k).zfill(2) + "_3d.png"))
            if path is not None:
                paths.append(path)
    return paths
