"""Shade a layout on the device: the ``--gan_shade`` path of the reference's ``test.py``.  Between the placed meshes (refine.py,
retrieve.py) and the 41-channel SPADE input (spade_input.py) the reference calls Blender (render/render_semantic_depth.py::render_test,
:152-377): it restores the boxes to metres, rests every retrieved model on the bottom of its box, draws up to ``Nsample = 5`` viewpoints
and keeps the first whose mean depth exceeds 0.7.  Here that is

  * ``shade_placement``   :153-234 in torch ops - float64 (the yardstick, bit for bit the reference's numpy on the host) or float32;
  * ``shade_viewpoint`` / ``shade_camera``   :355-360 and the camera matrices of the convention below;
  * ``ViewRenderer``      R rooms x V views: per-row affines in vectorised fp32 torch, ONE launch that places and projects every face of
    every view (csrc/shade_view.hip), ``sln_raster_forward`` at ``image_size = size``, one compose call (class bytes, depth in image row
    order, float64 sum / count of the depths below 1e5 per view), and the choice of :365-377 as a few ops on [R, V];
  * ``shade_layouts``     render -> ``InputBuilder(labels=, depth=)`` -> ``colorize`` per room; ``save_color`` writes the pictures;
  * ``views_torch``       the same steps in torch ops on any device and in either precision, with the caller's rasterizer: what the tests
    hold the kernels to, and what runs without a GPU.

Convention (stated here; Blender's own is not pinned - see DESIGN): the room's frame is y-up, the camera looks along its local -z with +y
up, ``R_wc = R_y(plane_angle) . R_x(-canonical_angle)`` (Blender's XYZ Euler with zero roll), the renderer's ``R = diag(1, -1, -1) . R_wc^T``
and ``t = -R . cam_coord`` as ``get_cam_mat`` forms them, ``K = [[S, 0, S/2], [0, S, S/2], [0, 0, 1]]`` with ``orig_size = S`` (a 50 mm lens
on a 50 mm sensor, vertical fit).

Differences from Blender that are not errors of this code: the shell is ``place_shell``'s (a dropped wall collapses instead of losing its
vertices), a face with a corner nearer than ``near`` is dropped whole instead of clipped, mask edges are not anti-aliased, and a view in
which no pixel is hit is not accepted (the reference would divide by zero at :373).
"""
import os

import numpy as np
import torch

from .. import _lib as L
from . import retrieve as RT
from . import refine as RF
from . import synthetic
from .spade_input import NYU40, colorize, to_uint8

NOT_IMPORTED = ("wall", "ceiling", "floor", "person", "door", "window", "curtain", "blinds")      # :240
N_SAMPLE = 5                 # :350
MIN_MEAN_DEPTH = 0.7         # :375
MEAN_BELOW = 1e5             # :370
EMPTY_Z = 1e10               # Blender's Z where nothing was hit
SNAP_Y = 0.02                # :168
_SHELL_LABEL = {"wall": 1 + NYU40.index("wall"), "floor": 1 + NYU40.index("floor"), "ceiling": 1 + NYU40.index("ceiling")}


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's arithmetic
# ------------------------------------------------------------------------------------------------------------------------------
def _host64(x):
    return x.dtype == torch.float64 and x.device.type == "cpu"


def _fn(name, x):
    """cos / sin / arctan.  For float64 on the host through numpy, element by element the reference's own calls: torch's vectorised
    double cos and sin differ from numpy's in the last bit for about 0.2 % of the arguments."""
    if _host64(x):
        return torch.from_numpy(np.asarray(getattr(np, name)(x.detach().numpy())))
    return getattr(torch, "atan" if name == "arctan" else name)(x)


def _rot_apply(rot, v):
    """rot [n, 3, 3] @ v [n, 3]: numpy's matmul for float64 on the host (its kernel does not add in the order of a written-out sum),
    a written-out sum elsewhere"""
    if _host64(rot):
        return torch.from_numpy(np.matmul(rot.detach().numpy(), v.detach().numpy()[:, :, None])[:, :, 0])
    return (rot[:, :, 0] * v[:, None, 0] + rot[:, :, 1] * v[:, None, 1]) + rot[:, :, 2] * v[:, None, 2]


def shade_placement(boxes, angles, objs, room_row, model_bbox):
    """:153-234 for row-concatenated rooms.  ``boxes`` [n, 6] room-normalised with every room's room row last (float64 or float32: the
    precision of everything that follows), ``angles`` [n] in bins of 2 pi / 24, ``objs`` [n] the row of ``model_bbox`` [M, 2, 3]
    (``bbox_min``, ``bbox_max`` of the model table) that holds the row's model - with one model per class the class index, with a
    retrieval ``class_ptr[class] + choice`` -, ``room_row`` [n] every row's room row.  -> dict of ``A`` [n, 3, 3] (``rot * scale``), ``tr`` [n, 3] (``trans``),
    ``center`` [n, 3], ``scaled_size`` [n, 3], ``boxes`` [n, 6] (restored to metres, heights snapped).  A room row's own entries mean
    nothing.  Unlike the refinement's placement (diff_render.py:76-159) the angle is not negated and the model rests on the bottom of
    its box (:228)."""
    dt = boxes.dtype
    bbox_min, bbox_max = model_bbox[objs.long(), 0], model_bbox[objs.long(), 1]
    room = boxes[room_row.long()]
    ext = room[:, 3:] - room[:, :3]                                         # :156-158
    lo, hi = boxes[:, :3] * ext, boxes[:, 3:] * ext                         # :160-165
    snap = lo[:, 1].abs() <= SNAP_Y                                         # :168-171
    hi_y = torch.where(snap, hi[:, 1] - lo[:, 1], hi[:, 1])
    lo_y = torch.where(snap, torch.zeros_like(lo[:, 1]), lo[:, 1])
    lo = torch.stack((lo[:, 0], lo_y, lo[:, 2]), 1)
    hi = torch.stack((hi[:, 0], hi_y, hi[:, 2]), 1)
    center, size = (hi + lo) / 2, hi - lo                                   # :210-211
    theta = angles.to(dt) * (2 * np.pi / 24)                                # :212
    msize, mcenter = bbox_max.to(dt) - bbox_min.to(dt), (bbox_min.to(dt) + bbox_max.to(dt)) / 2          # :221-222
    scale = (size / msize).min(dim=1).values                                # :223
    scaled = scale[:, None] * msize                                         # :226
    c, s = _fn("cos", theta), _fn("sin", theta)
    z, o = torch.zeros_like(c), torch.ones_like(c)
    rot = torch.stack((torch.stack((c, z, -s), 1), torch.stack((z, o, z), 1), torch.stack((s, z, c), 1)), 1)     # :227
    center = torch.stack((center[:, 0], center[:, 1] - (size[:, 1] - scaled[:, 1]) / 2, center[:, 2]), 1)        # :228
    tr = center - scale[:, None] * _rot_apply(rot, mcenter)                 # :229
    return dict(A=rot * scale[:, None, None], tr=tr, center=center, scaled_size=scaled, boxes=torch.cat((lo, hi), 1))


def shade_viewpoint(room_ext, t, jitter):
    """:355-360.  ``room_ext`` [..., 3] the room's extent in metres, ``t`` / ``jitter`` [...] the two uniform draws of a candidate view
    -> (cam_coord [..., 3], canonical_angle, plane_angle)"""
    pos = 0.2 + 0.6 * t
    cam = torch.stack((pos * room_ext[..., 0], 0.9 * room_ext[..., 1], room_ext[..., 2] + 0.4), -1)
    half = _fn("arctan", torch.full_like(pos, 25 / 50))
    canonical = np.pi / 2 - _fn("arctan", 0.4 / (0.9 * room_ext[..., 1])) - half
    canonical = canonical - jitter * 0.1
    plane = _fn("arctan", (cam[..., 0] - 0.5 * room_ext[..., 0]) / cam[..., 2]) * 1.1
    return cam, canonical, plane


def shade_camera(room_ext, t, jitter, size):
    """-> K [..., 3, 3], R [..., 3, 3], t [..., 3] of the module's convention for the viewpoint ``shade_viewpoint(room_ext, t, jitter)``"""
    cam, a, p = shade_viewpoint(room_ext, t, jitter)
    ca, sa, cp, sp = _fn("cos", a), _fn("sin", a), _fn("cos", p), _fn("sin", p)
    z = torch.zeros_like(ca)
    # R = diag(1, -1, -1) . (R_y(p) . R_x(-a))^T
    R = torch.stack((torch.stack((cp, z, -sp), -1), torch.stack((sp * sa, -ca, cp * sa), -1), torch.stack((-sp * ca, -sa, -cp * ca), -1)), -2)
    tv = -((R[..., 0] * cam[..., None, 0] + R[..., 1] * cam[..., None, 1]) + R[..., 2] * cam[..., None, 2])
    S = float(size)
    K = torch.zeros(*ca.shape, 3, 3, dtype=cam.dtype, device=cam.device)      # (filled by scalars: no host array crosses under a capture)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = S, S, S / 2, S / 2, 1.0
    return K, R.contiguous(), tv.contiguous()


def choose_view(sums, counts, min_mean_depth=MIN_MEAN_DEPTH):
    """:365-377 on [R, V]: ``sums`` float64 and ``counts`` int64 of the z-buffer entries below 1e5 -> (chosen [R] int64: the first view
    whose mean is ``> min_mean_depth``, 0 when none is; status [R] int32: 1 when none is).  A view without such an entry is not
    accepted (the reference divides by zero)."""
    V = sums.shape[1]
    mean = sums / counts.clamp(min=1).to(sums.dtype)
    ok = (counts > 0) & (mean > min_mean_depth)
    ar = torch.arange(V, device=sums.device)
    first = torch.where(ok, ar, V).min(dim=1).values
    none = first == V
    return torch.where(none, torch.zeros_like(first), first), none.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# the bank as the kernel reads it
# ------------------------------------------------------------------------------------------------------------------------------
class BankTables:
    """A ``MeshBank``'s models concatenated in the order of ``bank.table`` (class by class, table order within a class), plus the class
    bytes and the shell's topology.  Built once per (bank, device) and kept on the bank."""

    def __init__(self, bank, device):
        dev = torch.device(device)
        table = bank.table
        self.vocab = list(table.vocab)
        self.class_ptr_host = table.class_ptr_host.astype(np.int32)
        vs, fs, voff, foff, lo, hi, label = [], [], [0], [0], [], [], []
        for name in self.vocab:
            entries = bank.model_list(name) if name in bank.models else []
            if len(entries) != table.count(len(label)):
                raise ValueError("the bank's model table and its models disagree for class %r" % (name,))
            shown = name in NYU40 and name not in NOT_IMPORTED and len(entries) > 0
            label.append(1 + NYU40.index(name) if shown else 0)
            for e in entries:
                vs.append(e["v"].detach().float().cpu()); fs.append(e["f"].detach().to(torch.int32).cpu())
                voff.append(voff[-1] + vs[-1].shape[0]); foff.append(foff[-1] + fs[-1].shape[0])
                lo.append(e["bbox_min"].detach().float().cpu()); hi.append(e["bbox_max"].detach().float().cpu())
        self.M, self.Vtot, self.Ftot = len(vs), voff[-1], foff[-1]
        self.Fm = max([f.shape[0] for f in fs] + [1])
        self.voff_host, self.foff_host = np.asarray(voff, dtype=np.int32), np.asarray(foff, dtype=np.int32)
        # (one spare row each: an empty bank still has addresses, and the torch route's gathers something to clamp to)
        pad_v, pad_f, pad_b = torch.zeros(1, 3), torch.zeros(1, 3, dtype=torch.int32), torch.ones(1, 3)
        self.v = torch.cat(vs + [pad_v]).contiguous().to(dev)
        self.f = torch.cat(fs + [pad_f]).contiguous().to(dev)
        self.model_bbox = torch.stack((torch.cat([x[None] for x in lo] + [pad_b * 0]), torch.cat([x[None] for x in hi] + [pad_b])), 1).contiguous().to(dev)
        self.voff, self.foff = torch.from_numpy(self.voff_host).to(dev), torch.from_numpy(self.foff_host).to(dev)
        self.class_ptr = torch.from_numpy(self.class_ptr_host).to(dev)
        self.class_label = torch.tensor(label, dtype=torch.uint8, device=dev)
        topo = RF.shell_topology(bank, None)
        sf, sl, at = [], [], 0
        for name, nv, f in topo:
            sf.append(np.asarray(f, dtype=np.int64) + at); sl += [_SHELL_LABEL[name]] * int(f.shape[0]); at += nv
        self.Vs = at
        self.shell_f_host = np.ascontiguousarray(np.concatenate(sf).astype(np.int32)) if sf else np.zeros((0, 3), np.int32)
        self.Fs = int(self.shell_f_host.shape[0])
        self.shell_f = torch.from_numpy(np.concatenate([self.shell_f_host, np.zeros((1, 3), np.int32)])).to(dev)
        self.shell_label = torch.tensor(sl + [0], dtype=torch.uint8, device=dev)
        # the procedural shell is linear in the room's extent: unit quads (float64, place_shell's own numbers for a unit room)
        self.shell_unit = _unit_shell().to(dev) if getattr(bank, "shell", None) is None else None
        self.device = dev

    @classmethod
    def of(cls, bank, device):
        cache = bank.__dict__.setdefault("_shade_tables", {})
        key = str(torch.device(device))
        if key not in cache:
            cache[key] = cls(bank, device)
        return cache[key]


def _unit_shell():
    """the quads of ``place_shell``'s procedural shell for the room (1, 1, 1), float64 [Vs, 3]: every coordinate of that shell is ONE
    product of such a number with one extent (the other terms of its sum are exact zeros)"""
    quads = [((0, 0, 0), (0, 0, 1), (1, 0, 0)), ((0, 1, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 0), (1, 0, 0), (0, 1, 0)),
             ((0, 0, 0), (0, 1, 0), (0, 0, 1)), ((1, 0, 0), (0, 0, 1), (0, 1, 0))]               # floor, ceiling, back / left / right wall
    sv = [synthetic._grid_quad(np.array(p0, np.float64), np.array(du, np.float64), np.array(dv, np.float64), RF._SHELL_DIV)[0] for p0, du, dv in quads]
    return torch.from_numpy(np.concatenate(sv))


def procedural_shell(tables, room_ext):
    """``place_shell`` of the procedural shell for rooms [R, 3] on the extent's device: unit quads times the extent in float64, rounded
    to float32 once - ``place_shell``'s numbers bit for bit, without the room row on the host"""
    if tables.shell_unit is None:
        raise L.SlnError("a bank with shell meshes places its shell on the host: ViewRenderer.bind_shell(room extents) first")
    return (tables.shell_unit[None] * room_ext.double()[:, None, :]).float()


class Binding:
    """What follows the rooms' lengths ``rows`` only: the padded [R, N] gather of the row-concatenated arrays"""

    def __init__(self, rows, n_max, device):
        rows = [int(n) for n in rows]
        if not rows or min(rows) < 1:
            raise ValueError("rows: the length of every room (room row included), at least 1 each")
        self.rows, self.R = tuple(rows), len(rows)
        self.N = int(n_max) if n_max else max(rows)
        if max(rows) > self.N:
            raise ValueError("a room of %d rows in a renderer bound to %d" % (max(rows), self.N))
        row0 = np.concatenate([[0], np.cumsum(rows)])[:-1]
        last = row0 + np.asarray(rows) - 1
        k = np.arange(self.N)[None, :]
        valid = k < (np.asarray(rows)[:, None] - 1)                                  # object rows; the room row and the padding are not
        idx = np.where(valid, row0[:, None] + k, last[:, None])
        dev = torch.device(device)
        self.total = int(sum(rows))
        self.idx = torch.from_numpy(idx.astype(np.int64)).to(dev)                   # [R, N] -> row of the concatenated arrays
        self.valid = torch.from_numpy(valid).to(dev)
        self.last = torch.from_numpy(last.astype(np.int64)).to(dev)
        self.room_row = torch.from_numpy(np.repeat(last, rows).astype(np.int32)).to(dev)


def row_tables(tables, bind, boxes, angles, objs, choice, dtype):
    """Per row of the padded [R, N] layout, in torch ops on the arrays' device (no loop over objects, nothing read back):
    -> dict(A [R, N, 3, 3], tr [R, N, 3], row_model [R, N] int32, row_label [R, N] uint8, ext [R, 3])"""
    C = len(tables.vocab)
    o = objs.long()
    ok_cls = (o >= 0) & (o < C)
    oc = o.clamp(0, C - 1)
    ptr = tables.class_ptr.long()
    count = ptr[oc + 1] - ptr[oc]
    label = torch.where(ok_cls & (count > 0), tables.class_label[oc], torch.zeros_like(tables.class_label[oc]))
    pick = torch.zeros_like(o) if choice is None else choice.long().clamp(min=0)
    model = ptr[oc] + torch.minimum(pick, (count - 1).clamp(min=0))
    shown = (label > 0) & (torch.arange(o.numel(), device=o.device) != bind.room_row.long())
    model = torch.where(shown, model, torch.full_like(model, tables.M))            # (row M of the tables is the spare unit box)
    pl = shade_placement(boxes.to(dtype), angles, model, bind.room_row, tables.model_bbox.to(dtype))
    live = shown[bind.idx] & bind.valid
    room = boxes.to(dtype)[bind.last]
    return dict(A=pl["A"][bind.idx].contiguous(), tr=pl["tr"][bind.idx].contiguous(),
                row_model=torch.where(live, model[bind.idx], torch.full_like(bind.idx, -1)).to(torch.int32).contiguous(),
                row_label=torch.where(live, label[bind.idx], torch.zeros_like(label[bind.idx])).contiguous(),
                ext=room[:, 3:] - room[:, :3])


def place_project_torch(tables, rt, shell_v, K, Rm, t, size, near):
    """csrc/shade_view.hip's first kernel in torch ops, in the precision of ``rt``: -> faces_xyz [R * V, F, 3, 3], face_label [R, F]"""
    A, tr, row_model = rt["A"], rt["tr"], rt["row_model"].long()
    dt, dev = A.dtype, A.device
    R, N = row_model.shape
    V, Fm = K.shape[1], tables.Fm
    m = row_model.clamp(min=0)
    foff, voff = tables.foff.long(), tables.voff.long()
    j = torch.arange(Fm, device=dev)
    live = (row_model >= 0)[:, :, None] & (j < (foff[m + 1] - foff[m])[:, :, None])                       # [R, N, Fm]
    corner = tables.f[(foff[m][:, :, None] + j).clamp(max=max(tables.Ftot - 1, 0))].long()                # [R, N, Fm, 3]
    mv = tables.v.to(dt)[(voff[m][:, :, None, None] + corner).clamp(max=max(tables.Vtot - 1, 0))]         # [R, N, Fm, 3 corners, 3]
    Ab = A[:, :, None, None]                                                                              # [R, N, 1, 1, 3, 3]
    p = (Ab[..., 0] * mv[..., None, 0] + Ab[..., 1] * mv[..., None, 1]) + Ab[..., 2] * mv[..., None, 2] + tr[:, :, None, None]
    sp = shell_v.to(dt)[:, tables.shell_f[:tables.Fs].long()]                                             # [R, Fs, 3, 3]
    pts = torch.cat((p.reshape(R, N * Fm, 3, 3), sp), 1)[:, None]                                         # [R, 1, F, 3, 3]
    live = torch.cat((live.reshape(R, N * Fm), torch.ones(R, tables.Fs, dtype=torch.bool, device=dev)), 1)
    label = torch.cat((rt["row_label"][:, :, None].expand(R, N, Fm).reshape(R, N * Fm), tables.shell_label[:tables.Fs][None].expand(R, tables.Fs)), 1)
    label = torch.where(live, label, torch.zeros_like(label))
    Rb, tb, Kb = Rm[:, :, None, None], t[:, :, None, None], K[:, :, None, None]                           # [R, V, 1, 1, ...]
    cam = [(pts[..., 0] * Rb[..., i, 0] + pts[..., 1] * Rb[..., i, 1]) + pts[..., 2] * Rb[..., i, 2] + tb[..., i] for i in range(3)]
    os_, eps = float(size), 1e-9
    xh, yh = cam[0] / (cam[2] + eps), cam[1] / (cam[2] + eps)
    u = (xh * Kb[..., 0, 0] + yh * Kb[..., 0, 1]) + Kb[..., 0, 2]
    v = os_ - ((xh * Kb[..., 1, 0] + yh * Kb[..., 1, 1]) + Kb[..., 1, 2])
    out = torch.stack((2.0 * (u - os_ / 2.0) / os_, 2.0 * (v - os_ / 2.0) / os_, cam[2]), -1)             # [R, V, F, 3, 3]
    cull = ~live[:, None] | ~(cam[2] >= near).all(-1)
    out = torch.where(cull[..., None, None], torch.zeros_like(out), out)
    return out.reshape(R * V, -1, 3, 3).contiguous(), label.contiguous()


def compose_torch(face_index, depth, face_label, V):
    """csrc/shade_view.hip's compose in torch ops: maps [B, S, S] in raster order -> labels uint8 and depth float32 [B, S, S] in image
    row order, sum float64 [B] and count int64 [B] of the depths below 1e5"""
    B, F = face_index.shape[0], face_label.shape[1]
    fi = face_index.long()
    hit = (fi >= 0) & (fi < F)
    room = (torch.arange(B, device=fi.device) // V)[:, None, None]
    labels = torch.where(hit, face_label[room, fi.clamp(0, F - 1)], torch.zeros((), dtype=torch.uint8, device=fi.device))
    z = torch.where(hit, depth.float(), torch.full((), EMPTY_Z, dtype=torch.float32, device=fi.device))
    below = z < MEAN_BELOW
    sums = torch.where(below, z.double(), torch.zeros((), dtype=torch.float64, device=fi.device)).sum(dim=(1, 2))
    return torch.flip(labels, [1]).contiguous(), torch.flip(z, [1]).contiguous(), sums, below.sum(dim=(1, 2))


def vocab_lut(vocab, tables, device):
    """``objs`` index ``vocab`` (object_idx_to_name), the tables their own vocabulary: the map between them as a device table (None
    where the two are the same list)"""
    if vocab is None or list(vocab) == list(tables.vocab):
        return None
    own = {n: k for k, n in reversed(list(enumerate(tables.vocab)))}
    return torch.tensor([own.get(n, -1) for n in vocab] + [-1], dtype=torch.int64).to(device)


def _class_index(objs, lut):
    if lut is None:
        return objs
    o, n = objs.long(), lut.numel() - 1
    return lut[torch.where((o >= 0) & (o < n), o, torch.full_like(o, n))]


def views_torch(bank, boxes, angles, objs, rows, draws, rasterize, size=1024, views=N_SAMPLE, near=0.1, far=100.0, dtype=torch.float64,
                min_mean_depth=MIN_MEAN_DEPTH, vocab=None, n_max=None, shell_v=None, choice=None):
    """The route of ``ViewRenderer`` in torch ops on the arrays' device, in ``dtype``.  ``rasterize(faces float32 numpy [B, F, 3, 3],
    image_size, near, far) -> (face_index, weight, depth)`` numpy maps in raster order is the caller's rasterizer (the tests pass the C
    restatement the rasterizer kernels are held to).  ``draws`` [R, V, 2].  -> dict(labels [R, S, S] uint8, depth [R, S, S] float32,
    chosen [R], status [R], and of every view: faces_xyz, face_label, labels_all, depth_all, sums, counts, K, R, t)"""
    dev = boxes.device
    tables = BankTables.of(bank, dev)
    bind = Binding(rows, n_max, dev)
    objs = _class_index(objs, vocab_lut(vocab, tables, dev))
    if choice is None and bank.has_choice():
        choice = RT.retrieve_models_torch(boxes.float(), objs, bind.room_row, bank.table)
    rt = row_tables(tables, bind, boxes, angles, objs, choice, dtype)
    if shell_v is None:
        shell_v = procedural_shell(tables, rt["ext"].float())
    d = draws.to(device=dev, dtype=dtype)
    K, Rm, t = shade_camera(rt["ext"][:, None, :].expand(bind.R, views, 3), d[..., 0], d[..., 1], size)
    fxyz, flabel = place_project_torch(tables, rt, shell_v, K, Rm, t, size, near)
    fi, _, dep = rasterize(fxyz.float().cpu().numpy(), int(size), float(near), float(far))
    fi, dep = torch.from_numpy(np.ascontiguousarray(fi)).to(dev), torch.from_numpy(np.ascontiguousarray(dep)).to(dev)
    labels_all, depth_all, sums, counts = compose_torch(fi, dep, flabel, views)
    chosen, status = choose_view(sums.reshape(bind.R, views), counts.reshape(bind.R, views), min_mean_depth)
    pick = torch.arange(bind.R, device=dev) * views + chosen
    return dict(labels=labels_all[pick], depth=depth_all[pick], chosen=chosen, status=status, faces_xyz=fxyz, face_label=flabel, labels_all=labels_all,
                depth_all=depth_all, sums=sums, counts=counts, K=K, R=Rm, t=t, face_index=fi)


# ------------------------------------------------------------------------------------------------------------------------------
# the device route
# ------------------------------------------------------------------------------------------------------------------------------
def _stream(out):
    """the current stream of a device buffer; host tensors (the argument checks' tests: refused before any launch) have none"""
    return L.current_stream_ptr() if out.is_cuda else None


def place_project(tables, rt, shell_v, K, Rm, t, size, near, faces_xyz, face_label):
    """the bare launch of ``sln_view_place_project`` over the caller's buffers (contiguous float32 / int32 / uint8 on the device)"""
    R, N = rt["row_model"].shape
    V = int(K.shape[1])
    d = L.SlnViewPlace()
    P = lambda x: x.data_ptr()
    d.bank_v, d.bank_f, d.voff, d.foff = P(tables.v), P(tables.f), P(tables.voff), P(tables.foff)
    d.voff_host, d.foff_host = tables.voff_host.ctypes.data, tables.foff_host.ctypes.data
    d.A, d.tr, d.row_model, d.row_label = P(rt["A"]), P(rt["tr"]), P(rt["row_model"]), P(rt["row_label"])
    d.shell_v, d.shell_f, d.shell_label = P(shell_v), P(tables.shell_f), P(tables.shell_label)
    d.shell_f_host = tables.shell_f_host.ctypes.data if tables.Fs else None
    d.K, d.Rm, d.t = P(K), P(Rm), P(t)
    d.M, d.Vtot, d.Ftot, d.Fm, d.Vs, d.Fs, d.R, d.V, d.N = tables.M, tables.Vtot, tables.Ftot, tables.Fm, tables.Vs, tables.Fs, R, V, N
    d.orig_size, d.near = float(size), float(near)
    L.check(L.lib().sln_view_place_project(d, L.ptr(faces_xyz), L.ptr(face_label), _stream(faces_xyz)), "sln_view_place_project")


def compose(face_index, depth, face_label, V, workspace, labels, depth_out, sums, counts):
    """the bare ``sln_view_compose`` call (two launches) over the caller's buffers"""
    B, S, F = int(face_index.shape[0]), int(face_index.shape[1]), int(face_label.shape[1])
    L.check(L.lib().sln_view_compose(L.ptr(face_index), L.ptr(depth), L.ptr(face_label), B, int(V), F, S, L.ptr(workspace), L.ptr(labels),
                                     L.ptr(depth_out), L.ptr(sums), L.ptr(counts), _stream(labels)), "sln_view_compose")


class ViewRenderer:
    """The viewpoint render of ``batch`` rooms on the device.

        renderer = ViewRenderer(bank, size=1024, views=5, batch=R)
        labels, depth, chosen, status = renderer(boxes, angles, objs, rows)

    ``boxes`` [n, 6] float32 room-normalised, the rooms' rows concatenated with every room's room row last, ``angles`` [n] in bins,
    ``objs`` [n] class indices into ``vocab`` (``object_idx_to_name``; None: the bank's ``table_vocab()``), ``rows`` the R rooms' lengths
    (host integers).  ``draws`` [R, views, 2] are the viewpoints' uniforms (:355, :359), by default drawn on the device from ``generator``.
    With ``bank.has_choice()`` the models are those of ``retrieve.retrieve_models``.

    -> ``labels`` [R, S, S] uint8 (0: no class, 1 + c: NYU class c - what ``InputBuilder(labels=...)`` takes), ``depth`` [R, S, S]
    float32 (1e10 where nothing was hit), image row order; ``chosen`` [R] the accepted view, ``status`` [R] int32: 1 where no view was
    accepted (the reference returns None; the pictures are view 0's then).  These are the renderer's static buffers: the next call
    overwrites them.  Nothing is read back and there is no loop over objects; buffers that follow the rooms' lengths are built on the
    first call with those lengths (``bind``), so a captured call replays for rooms of the same lengths.  ``validate=True`` reads
    ``status`` after the call - one synchronisation - and raises ``ValueError``.  ``max_rows``: rows per room the buffers are sized for
    (default: the longest room of the first call)."""

    def __init__(self, bank, size=1024, views=N_SAMPLE, batch=1, near=0.1, far=100.0, min_mean_depth=MIN_MEAN_DEPTH, vocab=None, max_rows=None,
                 device="cuda", validate=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SlnError("ViewRenderer runs on the MI355X only (no CPU fallback); views_torch restates it for host tensors")
        self.bank, self.size, self.views, self.batch, self.near, self.far = bank, int(size), int(views), int(batch), float(near), float(far)
        self.min_mean_depth, self.vocab, self.max_rows, self.validate = float(min_mean_depth), vocab, max_rows, validate
        if self.size < 1 or self.views < 1 or self.batch < 1 or self.batch * self.views > 65535:
            raise ValueError("size, views and batch are positive, batch * views at most 65535")
        self.tables = BankTables.of(bank, self.device)
        self._bind, self._shell_v, self._lut = None, None, vocab_lut(vocab, self.tables, self.device)
        B, S, dev = self.batch * self.views, self.size, self.device
        lib = L.lib()
        self.face_index = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        self._weight = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
        self._raster_depth = torch.empty(B, S, S, dtype=torch.float32, device=dev)
        self.labels_all = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
        self.depth_all = torch.empty(B, S, S, dtype=torch.float32, device=dev)
        self.sums = torch.zeros(B, dtype=torch.float64, device=dev)
        self.counts = torch.zeros(B, dtype=torch.int64, device=dev)
        self._compose_ws = torch.empty(int(lib.sln_view_compose_workspace_bytes(B)) // 8, dtype=torch.int64, device=dev)
        self.labels = torch.empty(self.batch, S, S, dtype=torch.uint8, device=dev)
        self.depth = torch.empty(self.batch, S, S, dtype=torch.float32, device=dev)
        self.chosen = torch.zeros(self.batch, dtype=torch.int64, device=dev)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self._room0 = torch.arange(self.batch, device=dev) * self.views

    def bind(self, rows):
        """buffers that follow the rooms' lengths (set-up: allocates; not inside a capture)"""
        b = Binding(rows, self.max_rows, self.device)
        if b.R != self.batch:
            raise ValueError("%d rooms in a renderer of batch %d" % (b.R, self.batch))
        self.max_rows = b.N
        self.F = b.N * self.tables.Fm + self.tables.Fs
        B, dev = self.batch * self.views, self.device
        self.faces_xyz = torch.zeros(B, self.F, 3, 3, dtype=torch.float32, device=dev)
        self.face_label = torch.zeros(self.batch, self.F, dtype=torch.uint8, device=dev)
        self._raster_ws = torch.empty(int(L.lib().sln_raster_workspace_bytes(B, self.F)), dtype=torch.uint8, device=dev)
        self._bind = b
        return b

    def bind_shell(self, room_exts, shell=None):
        """a bank with shell meshes: ``place_shell`` per room on the host, once (``room_exts``: R triples of host floats)"""
        self._shell_v = torch.stack([RF.place_shell(self.bank, e, shell) for e in room_exts]).contiguous().to(self.device)

    def __call__(self, boxes, angles, objs, rows, draws=None, generator=None):
        dev = self.device
        if not torch.is_tensor(boxes) or boxes.device != self.labels.device or boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 6:
            raise ValueError("boxes: a float32 tensor [n, 6] on %s expected" % self.labels.device)
        rows = tuple(int(n) for n in rows)
        bind = self._bind if self._bind is not None and self._bind.rows == rows else self.bind(rows)
        if boxes.shape[0] != bind.total or angles.numel() != bind.total or objs.numel() != bind.total:
            raise ValueError("boxes, angles and objs name the %d rows of `rows`" % bind.total)
        objs = _class_index(objs.to(dev).reshape(-1), self._lut)
        choice = None
        if self.bank.has_choice():
            choice = RT.retrieve_models(boxes.contiguous(), objs.to(torch.int32), bind.room_row, self.bank.table)
        rt = row_tables(self.tables, bind, boxes, angles.to(dev).reshape(-1), objs, choice, torch.float32)
        shell_v = self._shell_v if self._shell_v is not None else procedural_shell(self.tables, rt["ext"])
        if draws is None:
            draws = torch.rand(self.batch, self.views, 2, device=dev, generator=generator)
        d = draws.to(device=dev, dtype=torch.float32)
        if tuple(d.shape) != (self.batch, self.views, 2):
            raise ValueError("draws: [%d, %d, 2] expected" % (self.batch, self.views))
        K, Rm, t = shade_camera(rt["ext"][:, None, :].expand(self.batch, self.views, 3), d[..., 0], d[..., 1], self.size)
        place_project(self.tables, rt, shell_v.contiguous(), K, Rm, t, self.size, self.near, self.faces_xyz, self.face_label)
        B = self.batch * self.views
        L.check(L.lib().sln_raster_forward(L.ptr(self.faces_xyz), B, self.F, self.size, self.near, self.far, L.ptr(self._raster_ws),
                                           L.ptr(self.face_index), L.ptr(self._weight), L.ptr(self._raster_depth), L.current_stream_ptr()),
                "sln_raster_forward")
        compose(self.face_index, self._raster_depth, self.face_label, self.views, self._compose_ws, self.labels_all, self.depth_all, self.sums,
                self.counts)
        chosen, status = choose_view(self.sums.reshape(self.batch, self.views), self.counts.reshape(self.batch, self.views), self.min_mean_depth)
        self.chosen.copy_(chosen); self.status.copy_(status)
        pick = self._room0 + self.chosen
        torch.index_select(self.labels_all, 0, pick, out=self.labels)
        torch.index_select(self.depth_all, 0, pick, out=self.depth)
        if self.validate:
            _raise_unaccepted(self.status)
        return self.labels, self.depth, self.chosen, self.status


def _raise_unaccepted(status):
    bad = status.cpu().nonzero().flatten().tolist()
    if bad:
        raise ValueError("no viewpoint of room(s) %s has a mean depth above the threshold (the reference prints 'Failed to sample good view "
                         "point' and returns None)" % bad)


def shade_layouts(generator, renderer, builder, boxes, angles, objs, rows, num_z, draws=None, rng=None, validate=False):
    """``--gan_shade`` for R rooms: the viewpoint render, the 41-channel input of every room (``builder``: a batch-1
    ``InputBuilder(size, size)``) and ``num_z`` shaded images of it from ``generator`` (a ``SPADEGenerator4``).  ``rng``: the torch
    generator of the viewpoint draws and the z vectors.  -> (uint8 [R, num_z, 256, 256, 3], status [R]).  Nothing is read back unless
    ``validate`` is set: then a room without an accepted view raises ``ValueError``; otherwise it is shaded from view 0 and flagged."""
    if builder.batch != 1 or (builder.H, builder.W) != (renderer.size, renderer.size):
        raise ValueError("a batch-1 builder of the renderer's size expected")
    labels, depth, _, status = renderer(boxes, angles, objs, rows, draws=draws, generator=rng)
    if validate:
        _raise_unaccepted(status)
    out = [to_uint8(colorize(generator, builder(depth[r], labels=labels[r]), num_z, rng)) for r in range(renderer.batch)]
    return torch.stack(out), status


def save_color(data, folder_name='./images', prefix='target'):
    """testing/test_SPADE_shade.py::save_color (:16-27): ``data[0]`` [3, S, S] in [-1, 1] -> ``<prefix>_color.png``"""
    from .scene_pictures import _folder, _write
    _folder(folder_name)
    return _write(to_uint8(data[0:1])[0], os.path.join(folder_name, prefix + "_color.png"))
