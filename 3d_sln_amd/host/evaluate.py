"""Layout evaluation on the device - the ``--measure_acc_l1_std`` mode of the reference's ``test.py``
(``testing/test_acc_mean_std.py:10-125``: ``get_acc_l1`` and ``get_std``) without a host round trip per batch.

  * ``relation_acc``  - scene_graph_acc (testing/test_utils.py:135-152: restore_box + compute_rel + compare by name) of S layouts
    in one launch (sln_layout_relation_acc), with an optional predicate confusion table;
  * ``layout_l1``     - F.l1_loss of S layouts against the ground truth (sln_layout_l1);
  * ``layout_spread`` - the get_std figures of one batch from its Nsample decodes (sln_layout_spread);
  * ``baselines``     - the random and perturbed layouts of get_acc_l1 (sln_layout_baselines), draws injected or drawn on the device;
  * ``measure_acc_l1_std`` - the whole mode: the nine figures the reference prints, read back once at the end;
  * ``cuboid_iou``    - the rotated-cuboid 3-D IoU of S layouts against the ground truth (testing/test_render_refine.py:78-116,360-368,
    testing/test_utils.py:7-40) with per-room means (sln_layout_cuboid_iou) - the figure of the refinement table;
  * ``layout_overlap`` - how much of a layout's furniture interpenetrates: intersection volume and pair count (sln_layout_overlap);
  * ``overlap_penalty`` - that volume per room as a differentiable loss term (sln_layout_overlap_penalty).

The ``*_torch`` functions restate each kernel in torch ops for CPU tensors (the host-side tests), as ``sampling.layout_heatmap``
does for the heat-map kernel.
"""
import ctypes as C
import pickle

import numpy as np
import torch

from .. import _lib
from . import sampling as _S

RELATIONSHIPS = _S.RELATIONSHIPS          # compute_rel's relation order (= the graph builder's predicate indices)
_IN_ROOM, _ON, _INSIDE, _SURROUND = 0, 15, 5, 6
_LEFT, _RIGHT, _BEHIND, _FRONT, _LEFT_T, _RIGHT_T, _FRONT_T, _BEHIND_T = 1, 2, 3, 4, 7, 8, 9, 10
NONE = 16                                 # confusion column of compute_rel returning None


# ------------------------------------------------------------------------------------------------------------------------------
# vocabulary
# ------------------------------------------------------------------------------------------------------------------------------
def room_class(vocab):
    """index of '__room__' in vocab['object_idx_to_name'] (restore_box and compute_rel test the NAME, test_utils.py:122, utils.py:41)"""
    return list(vocab["object_idx_to_name"]).index("__room__")


def relation_table(vocab):
    """[16] int32: relation r of compute_rel -> the index of the predicate named RELATIONSHIPS[r] in vocab['pred_idx_to_name'], -1 where
    the vocabulary lacks the name (such triples never match: test_utils.py:148-151 compares names)."""
    names = list(vocab["pred_idx_to_name"])
    tab = []
    for r in RELATIONSHIPS:
        hits = [i for i, n in enumerate(names) if n == r]
        if len(hits) > 1:
            raise ValueError("pred_idx_to_name names %r more than once" % r)
        tab.append(hits[0] if hits else -1)
    return torch.tensor(tab, dtype=torch.int32)


def _check_layouts(boxes):
    if boxes.dim() != 3 or boxes.shape[2] != 6:
        raise ValueError("layouts must be [S, O, 6] (box_dim 6), got %s" % (tuple(boxes.shape),))


# ------------------------------------------------------------------------------------------------------------------------------
# device entry points
# ------------------------------------------------------------------------------------------------------------------------------
def relation_acc(boxes, objs, triples, room_cls, table, good=None, confusion=None):
    """boxes [S, O, 6] (not modified), objs [O], triples [T, 3] on the device -> good [S] int64 (+= into ``good``) and, when
    ``confusion`` is True or a [S, 16, 17] int64 tensor, the confusion table (+= into it)."""
    _check_layouts(boxes)
    S, O, bd = boxes.shape
    dev = boxes.device
    b = boxes.contiguous()
    objs = objs.to(torch.int64).contiguous()
    triples = triples.to(torch.int64).reshape(-1, 3).contiguous()
    if good is None:
        good = torch.zeros(S, dtype=torch.int64, device=dev)
    if confusion is True:
        confusion = torch.zeros(S, 16, 17, dtype=torch.int64, device=dev)
    elif confusion is False:
        confusion = None
    tab = (C.c_int * 16)(*[int(x) for x in table])
    _lib.check(_lib.lib().sln_layout_relation_acc(_lib.ptr(b), S, O, bd, _lib.ptr(objs), _lib.ptr(triples), triples.shape[0], int(room_cls), tab,
                                                  _lib.ptr(good), _lib.ptr(confusion), _lib.current_stream_ptr()), "sln_layout_relation_acc")
    return good, confusion


def layout_l1(boxes, gt, out=None):
    """boxes [S, O, 6], gt [O, 6] -> [S] float64 (+= into ``out``): F.l1_loss(boxes[s], gt)"""
    _check_layouts(boxes)
    S, O, bd = boxes.shape
    b, g = boxes.contiguous(), gt.float().contiguous()
    if g.shape != (O, 6):
        raise ValueError("gt must be [O, 6]")
    out = torch.zeros(S, dtype=torch.float64, device=boxes.device) if out is None else out
    _lib.check(_lib.lib().sln_layout_l1(_lib.ptr(b), S, O, bd, _lib.ptr(g), _lib.ptr(out), _lib.current_stream_ptr()), "sln_layout_l1")
    return out


def layout_spread(boxes, angle_bins, out=None):
    """boxes [S, O, 6] (un-restored decodes), angle_bins [S, O] -> [3] float64 (+= into ``out``): mean angle / position / size std"""
    _check_layouts(boxes)
    S, O, bd = boxes.shape
    b, a = boxes.contiguous(), angle_bins.to(torch.int64).contiguous()
    out = torch.zeros(3, dtype=torch.float64, device=boxes.device) if out is None else out
    _lib.check(_lib.lib().sln_layout_spread(_lib.ptr(b), _lib.ptr(a), S, O, bd, _lib.ptr(out), _lib.current_stream_ptr()), "sln_layout_spread")
    return out


def baselines(gt, objs, room_cls, uniforms=None, normals=None, key=None, out=None):
    """gt [O, 6] -> [2, O, 6]: random_scene and the perturbed layout.  Draws: ``uniforms`` / ``normals`` [O, 3] (float32, row-indexed)
    or ``key`` (int64 [2] on the device; default: two words from torch's device generator)."""
    if gt.dim() != 2 or gt.shape[1] != 6:
        raise ValueError("gt must be [O, 6] (box_dim 6)")
    O = gt.shape[0]
    dev = gt.device
    g, o = gt.float().contiguous(), objs.to(torch.int64).contiguous()
    out = torch.empty(2, O, 6, dtype=torch.float32, device=dev) if out is None else out
    if uniforms is not None:
        u, n = uniforms.float().contiguous(), normals.float().contiguous()
        key = None
    else:
        u = n = None
        if key is None:
            key = torch.randint(-2 ** 62, 2 ** 62, (2,), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().sln_layout_baselines(_lib.ptr(g), _lib.ptr(o), O, 6, int(room_cls), _lib.ptr(u), _lib.ptr(n), _lib.ptr(key), _lib.ptr(out),
                                               _lib.current_stream_ptr()), "sln_layout_baselines")
    return out


DO_NOT_VIS = ("wall", "ceiling", "floor", "person", "door", "window", "curtain", "blinds")      # testing/test_render_refine.py:16
MAX_ROOM_ROWS = 1024                      # rows of one room sln_layout_overlap stages at once


def visible_rows(objs, vocab_names):
    """[O] bool: the rows get_boxes keeps (test_render_refine.py:87-89: the class name is not in do_not_vis) - room rows included"""
    names = list(vocab_names)
    keep = torch.tensor([n not in DO_NOT_VIS for n in names], dtype=torch.bool, device=objs.device)
    return keep[objs.to(torch.int64)]


def room_rows(objs, room_cls):
    """[O] int32: for every row the index of its room row - the first row of class ``room_cls`` at or behind it, the last row of its
    room (restore_box, test_utils.py:119-132; get_boxes' ``input_boxes[-1]`` for a single room); -1 behind the last room row"""
    is_room = (objs.to(torch.int64) == int(room_cls)).cpu().tolist()
    out, j = [], -1
    for i in range(len(is_room) - 1, -1, -1):
        if is_room[i]:
            j = i
        out.append(j)
    return torch.tensor(out[::-1], dtype=torch.int32, device=objs.device)


def _room_ids(room_of_row):
    """[O] int32 ordinal of every row's room, and the number of rooms (host side: one read of the table)"""
    r = room_of_row.cpu().to(torch.int64)
    uniq, inv = torch.unique(r, sorted=True, return_inverse=True)
    return inv.to(torch.int32).to(room_of_row.device), int(uniq.numel())


def _check_rooms(room_of_row, O):
    r = room_of_row.cpu().to(torch.int64)
    if r.shape != (O,) or bool((r < torch.arange(O)).any()) or bool((r >= O).any()) or bool((r[1:] < r[:-1]).any()) or bool((r[r] != r).any()):
        raise ValueError("room_of_row must be [O]: for every row the index of the last row of its room (rows of a room consecutive)")
    return r


def cuboid_iou(boxes, angles, gt_boxes, gt_angles, room_of_row, visible, room_id=None, n_rooms=None, want_rows=True, mean=None):
    """boxes [S, O, 6], angles [S, O] (float bins) against gt_boxes [O, 6], gt_angles [O] -> (iou [S, O] float32 or None,
    mean [S, n_rooms] float64, += into ``mean``): get_iou_cuboid of every row, averaged over the visible rows of every room."""
    _check_layouts(boxes)
    S, O, _ = boxes.shape
    dev = boxes.device
    if angles.shape != (S, O) or gt_boxes.shape != (O, 6) or gt_angles.shape != (O,) or visible.shape != (O,):
        raise ValueError("angles must be [S, O], gt_boxes [O, 6], gt_angles and visible [O]")
    _check_rooms(room_of_row, O)
    if room_id is None:
        room_id, n_rooms = _room_ids(room_of_row)
    b, a = boxes.float().contiguous(), angles.float().contiguous()
    g, ga = gt_boxes.float().contiguous(), gt_angles.float().contiguous()
    rr, vis, rid = room_of_row.to(torch.int32).contiguous(), visible.to(torch.uint8).contiguous(), room_id.to(torch.int32).contiguous()
    iou = torch.empty(S, O, dtype=torch.float32, device=dev) if want_rows else None
    mean = torch.zeros(S, int(n_rooms), dtype=torch.float64, device=dev) if mean is None else mean
    if mean.shape != (S, int(n_rooms)) or mean.dtype != torch.float64:
        raise ValueError("mean must be [S, n_rooms] float64")
    for s0 in range(0, S, 65535):                       # (the layout index is a grid axis)
        n = min(65535, S - s0)
        _lib.check(_lib.lib().sln_layout_cuboid_iou(_lib.ptr(b[s0:]), _lib.ptr(a[s0:]), _lib.ptr(g), _lib.ptr(ga), _lib.ptr(rr), _lib.ptr(vis), _lib.ptr(rid),
                                                    int(n_rooms), n, O, _lib.ptr(iou[s0:]) if want_rows else None, _lib.ptr(mean[s0:]),
                                                    _lib.current_stream_ptr()), "sln_layout_cuboid_iou")
    return iou, mean


def layout_overlap(boxes, angles, room_of_row, visible, thresh=0.0, vol=None, pairs=None):
    """boxes [S, O, 6], angles [S, O] -> (vol [S] float64, pairs [S] int64), both +=: over the pairs of visible rows of the same room,
    the summed intersection volume and the number of pairs whose IoU exceeds ``thresh``"""
    _check_layouts(boxes)
    S, O, _ = boxes.shape
    dev = boxes.device
    if angles.shape != (S, O) or visible.shape != (O,):
        raise ValueError("angles must be [S, O], visible [O]")
    r = _check_rooms(room_of_row, O)
    if O and int(torch.bincount(r).max()) > MAX_ROOM_ROWS:
        raise ValueError("a room of more than %d rows" % MAX_ROOM_ROWS)
    b, a = boxes.float().contiguous(), angles.float().contiguous()
    rr, vis = room_of_row.to(torch.int32).contiguous(), visible.to(torch.uint8).contiguous()
    vol = torch.zeros(S, dtype=torch.float64, device=dev) if vol is None else vol
    pairs = torch.zeros(S, dtype=torch.int64, device=dev) if pairs is None else pairs
    _lib.check(_lib.lib().sln_layout_overlap(_lib.ptr(b), _lib.ptr(a), _lib.ptr(rr), _lib.ptr(vis), S, O, float(thresh), _lib.ptr(vol), _lib.ptr(pairs),
                                             _lib.current_stream_ptr()), "sln_layout_overlap")
    return vol, pairs


def collide_rows(objs, vocab_names, room_cls):
    """[O] bool: the rows whose interpenetration ``overlap_penalty`` counts by default - the class is not in DO_NOT_VIS and the row is
    not a room row (``visible_rows`` keeps room rows; a room row's cuboid is the room itself)"""
    return visible_rows(objs, vocab_names) & (objs.to(torch.int64) != int(room_cls))


def _check_penalty_arguments(boxes, angles, room_of_row, collide):
    _check_layouts(boxes)
    S, O, _ = boxes.shape
    if angles.shape != (S, O) or collide.shape != (O,):
        raise ValueError("angles must be [S, O], collide [O]")
    r = _check_rooms(room_of_row, O)
    if O and int(torch.bincount(r).max()) > MAX_ROOM_ROWS:
        raise ValueError("a room of more than %d rows" % MAX_ROOM_ROWS)


def overlap_penalty_launch(boxes, angles, room_of_row, collide, room_id, n_rooms, weight=1.0, accumulate=False, penalty=None, grad_boxes=None,
                           grad_angles=None):
    """the one sln_layout_overlap_penalty launch on prepared device tensors (float32 contiguous layouts, int32 tables, uint8 ``collide``)
    -> (penalty [S, n_rooms] float64 written, grad_boxes [S, O, 6], grad_angles [S, O] = weight * d penalty, written or added onto)"""
    S, O, _ = boxes.shape
    dev = boxes.device
    penalty = torch.empty(S, int(n_rooms), dtype=torch.float64, device=dev) if penalty is None else penalty
    if grad_boxes is None:
        grad_boxes, grad_angles = torch.empty(S, O, 6, dtype=torch.float32, device=dev), torch.empty(S, O, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().sln_layout_overlap_penalty(_lib.ptr(boxes), _lib.ptr(angles), _lib.ptr(room_of_row), _lib.ptr(collide), _lib.ptr(room_id),
                                                     int(n_rooms), S, O, float(weight), int(bool(accumulate)), _lib.ptr(penalty), _lib.ptr(grad_boxes),
                                                     _lib.ptr(grad_angles), _lib.current_stream_ptr()), "sln_layout_overlap_penalty")
    return penalty, grad_boxes, grad_angles


class _OverlapPenaltyFn(torch.autograd.Function):
    """penalty [S, n_rooms] float64 of boxes [S, O, 6] / angles [S, O]: the forward computes the gradients too (one launch on the device,
    the torch restatement on CPU tensors), the backward scales every row by its room's incoming gradient"""

    @staticmethod
    def forward(ctx, boxes, angles, room_of_row, collide, room_id, n_rooms):
        if boxes.is_cuda:
            b, a = boxes.detach().float().contiguous(), angles.detach().float().contiguous()
            pen, gb, ga = overlap_penalty_launch(b, a, room_of_row.to(torch.int32).contiguous(), collide.to(torch.uint8).contiguous(),
                                                 room_id.to(torch.int32).contiguous(), n_rooms)
        else:
            pen, gb, ga = overlap_penalty_torch(boxes.detach(), angles.detach(), room_of_row, collide, room_id=room_id, n_rooms=n_rooms)
        ctx.save_for_backward(gb, ga, room_id.to(torch.int64))
        ctx.dtypes = (boxes.dtype, angles.dtype)
        return pen

    @staticmethod
    def backward(ctx, gout):
        gb, ga, rid = ctx.saved_tensors
        up = gout[:, rid].to(gb.dtype)                                                   # [S, O]: the row's room's upstream gradient
        return (gb * up[..., None]).to(ctx.dtypes[0]), (ga * up).to(ctx.dtypes[1]), None, None, None, None


def overlap_penalty(boxes, angles, room_of_row, collide, room_id=None, n_rooms=None):
    """boxes [S, O, 6], angles [S, O] (float bins) -> penalty [S, n_rooms] float64, differentiable in both: per room the summed
    intersection volume of the pairs of rows with ``collide`` != 0 - what ``layout_overlap`` reports, as a loss term.  The
    room rows' extents are constants and a room row's gradient is 0.  One sln_layout_overlap_penalty launch on the device;
    ``overlap_penalty_torch`` on CPU tensors."""
    _check_penalty_arguments(boxes, angles, room_of_row, collide)
    if room_id is None:
        room_id, n_rooms = _room_ids(room_of_row)
    return _OverlapPenaltyFn.apply(boxes, angles, room_of_row, collide, room_id, int(n_rooms))


# ------------------------------------------------------------------------------------------------------------------------------
# torch restatements (CPU tensors)
# ------------------------------------------------------------------------------------------------------------------------------
def _shoelace(q):
    """signed area of rings q [..., n, 2]"""
    x, y = q[..., 0], q[..., 1]
    return 0.5 * (x * torch.roll(y, -1, -1) - torch.roll(x, -1, -1) * y).sum(-1)


def quad_intersection_area_torch(a, b):
    """area of quad a ^ quad b, [..., 4, 2] each (convex, any winding): Sutherland-Hodgman of a against the edges of b on masks -
    the device function of csrc/layout_iou.hip, statement for statement"""
    a, b = torch.broadcast_tensors(a, b)
    flip = lambda q: torch.where((_shoelace(q) < 0)[..., None, None], q[..., [0, 3, 2, 1], :], q)
    a, b = flip(a), flip(b)
    shape = a.shape[:-2]
    P = torch.zeros(shape + (8, 2), dtype=a.dtype)
    P[..., :4, :] = a
    n = torch.full(shape, 4, dtype=torch.int64)
    slots = torch.arange(8)
    for e in range(4):
        b0, ed = b[..., e, :], b[..., (e + 1) % 4, :] - b[..., e, :]
        d = ed[..., None, 0] * (P[..., 1] - b0[..., None, 1]) - ed[..., None, 1] * (P[..., 0] - b0[..., None, 0])
        out = torch.zeros_like(P)
        m = torch.zeros_like(n)
        for k in range(8):
            wrap = (k + 1) >= n
            kn = (k + 1) % 8
            nxt = torch.where(wrap[..., None], P[..., 0, :], P[..., kn, :])
            dn = torch.where(wrap, d[..., 0], d[..., kn])
            cur, dc = P[..., k, :], d[..., k]
            live = k < n
            in_c, in_n = dc >= 0, dn >= 0
            put_c = live & in_c
            put_x = live & (in_c != in_n) & ~torch.isnan(dc) & ~torch.isnan(dn)
            t = dc / (dc - dn)
            ip = cur + t[..., None] * (nxt - cur)
            w = (put_c[..., None] & (slots == m[..., None]))[..., None]
            out = torch.where(w, cur[..., None, :], out)
            m = m + put_c.long()
            w = (put_x[..., None] & (slots == m[..., None]))[..., None]
            out = torch.where(w, ip[..., None, :], out)
            m = m + put_x.long()
        n, P = m.clamp(max=8), out
    k = slots.expand(shape + (8,))
    nxt_i = torch.where(k + 1 >= n[..., None], torch.zeros_like(k), (k + 1) % 8)
    Pn = torch.gather(P, -2, nxt_i[..., None].expand(shape + (8, 2)))
    term = P[..., 0] * Pn[..., 1] - Pn[..., 0] * P[..., 1]
    return (0.5 * torch.where(k < n[..., None], term, torch.zeros_like(term)).sum(-1)).abs()


def cuboids_torch(boxes, angles, room_of_row, dtype=torch.float64):
    """get_boxes (test_render_refine.py:90-110) of boxes [..., O, 6] / angles [..., O] -> (ring [..., O, 4, 2] in (x, z), h0, h1)"""
    b, ang = boxes.to(dtype), angles.to(dtype)
    rr = room_of_row.to(torch.int64).clamp(min=0)
    ext = b[..., rr, 3:6]
    mn, mx = b[..., 0:3] * ext, b[..., 3:6] * ext
    ctr = (mx + mn) / 2
    mn, mx = mn - ctr, mx - ctr
    theta = -ang * float(np.float32(2.0 * float(np.pi) / 24.0))
    c, s = torch.cos(theta), torch.sin(theta)
    xs = torch.stack([mn[..., 0], mn[..., 0], mx[..., 0], mx[..., 0]], -1)
    zs = torch.stack([mn[..., 2], mx[..., 2], mx[..., 2], mn[..., 2]], -1)
    ring = torch.stack([c[..., None] * xs + s[..., None] * zs + ctr[..., None, 0], -s[..., None] * xs + c[..., None] * zs + ctr[..., None, 2]], -1)
    return ring, mn[..., 1] + ctr[..., 1], mx[..., 1] + ctr[..., 1]


def _pair_iou(ra, h0a, h1a, rb, h0b, h1b):
    inter = quad_intersection_area_torch(ra, rb) * (torch.minimum(h1a, h1b) - torch.maximum(h0a, h0b)).clamp(min=0)
    va, vb = _shoelace(ra).abs() * (h1a - h0a), _shoelace(rb).abs() * (h1b - h0b)
    return inter / (va + vb - inter + 1e-5), inter


def cuboid_iou_torch(boxes, angles, gt_boxes, gt_angles, room_of_row, visible=None, room_id=None, n_rooms=None, dtype=torch.float64):
    """cuboid_iou as torch ops in ``dtype`` -> (iou [S, O], mean [S, n_rooms]; NaN for a room without a visible row)"""
    S, O, _ = boxes.shape
    rp, p0, p1 = cuboids_torch(boxes, angles, room_of_row, dtype)
    rg, g0, g1 = cuboids_torch(gt_boxes, gt_angles, room_of_row, dtype)
    iou, _ = _pair_iou(rg[None], g0[None], g1[None], rp, p0, p1)
    if visible is None:
        visible = torch.ones(O, dtype=torch.bool)
    if room_id is None:
        room_id, n_rooms = _room_ids(room_of_row)
    mean = torch.full((S, int(n_rooms)), float("nan"), dtype=dtype)
    for r in range(int(n_rooms)):
        rows = torch.nonzero((room_id == r) & visible.bool()).flatten()
        if rows.numel():
            mean[:, r] = iou[:, rows].sum(1) / rows.numel()
    return iou, mean


def layout_overlap_torch(boxes, angles, room_of_row, visible, thresh=0.0, dtype=torch.float64):
    """layout_overlap as torch ops -> (vol [S], pairs [S] int64, iou of every counted pair [S, n_pairs])"""
    S, O, _ = boxes.shape
    ring, h0, h1 = cuboids_torch(boxes, angles, room_of_row, dtype)
    vis = visible.bool()
    i, j = torch.triu_indices(O, O, 1)
    ok = (room_of_row[i] == room_of_row[j]) & vis[i] & vis[j]
    i, j = i[ok], j[ok]
    iou, inter = _pair_iou(ring[:, i], h0[:, i], h1[:, i], ring[:, j], h0[:, j], h1[:, j])
    return inter.sum(1), (iou > thresh).sum(1), iou


def quad_area_grad_torch(a, b):
    """d quad_intersection_area(a, b) / d a [..., 4, 2], b fixed (quad_area_grad of csrc/layout_iou.hip): of the boundary of a ^ b only
    the pieces of a's edges inside b move with a's vertices to first order.  Both rings in counter-clockwise order as the area
    function brings them; edge p -> q of a (d = q - p) clipped to [s0, s1] of [0, 1] by b's four half planes (the inside rule >= 0),
    w = (s1^2 - s0^2) / 2: dA/dp += (d.y, -d.x) ((s1 - s0) - w), dA/dq += (d.y, -d.x) w.  No quotient is formed where it is not used."""
    a, b = torch.broadcast_tensors(a, b)
    perm = [0, 3, 2, 1]
    fa = (_shoelace(a) < 0)[..., None, None]
    p = torch.where(fa, a[..., perm, :], a)
    b0 = torch.where((_shoelace(b) < 0)[..., None, None], b[..., perm, :], b)
    q, ed = torch.roll(p, -1, -2), torch.roll(b0, -1, -2) - b0
    edge = lambda v: ed[..., None, :, 0] * (v[..., :, None, 1] - b0[..., None, :, 1]) - ed[..., None, :, 1] * (v[..., :, None, 0] - b0[..., None, :, 0])
    f0, f1 = edge(p), edge(q)                                                            # [..., edge of a, edge of b]
    in0, in1 = f0 >= 0, f1 >= 0
    cross = (in0 != in1) & ~torch.isnan(f0) & ~torch.isnan(f1)
    one, zero = torch.ones_like(f0), torch.zeros_like(f0)
    t = torch.where(cross, f0, zero) / torch.where(cross, f0 - f1, one)
    s1 = torch.where(cross & in0, t, one).min(-1).values
    s0 = torch.where(cross & ~in0, t, zero).max(-1).values
    live = ~(~(in0 & in1) & ~cross).any(-1) & (s1 > s0)
    w = (s1 * s1 - s0 * s0) / 2
    d = q - p
    n = torch.stack([d[..., 1], -d[..., 0]], -1)
    off = torch.zeros_like(w)
    g = n * torch.where(live, (s1 - s0) - w, off)[..., None] + torch.roll(n * torch.where(live, w, off)[..., None], 1, -2)
    return torch.where(fa, g[..., perm, :], g)


def overlap_penalty_torch(boxes, angles, room_of_row, collide, dtype=torch.float64, room_id=None, n_rooms=None):
    """The definition of ``overlap_penalty`` in torch ops on CPU tensors -> (penalty [S, n_rooms], grad_boxes [S, O, 6],
    grad_angles [S, O]) in ``dtype``, NaN-safe: V_ij = A(ring_i, ring_j) * max(0, min(h1) - max(h0)) over the pairs of colliding rows of
    one room; d A by ``quad_area_grad_torch``; the height factor's derivative with one half per row on an exact tie; a pair whose height
    overlap is <= 0 contributes nothing; the chain through get_boxes' expressions with the room row's extent a constant."""
    _check_penalty_arguments(boxes, angles, room_of_row, collide)
    S, O, _ = boxes.shape
    if room_id is None:
        room_id, n_rooms = _room_ids(room_of_row)
    b, ang = boxes.detach().to(dtype), angles.detach().to(dtype)
    rr, rid = room_of_row.to(torch.int64), room_id.to(torch.int64)
    ring, h0, h1 = cuboids_torch(b, ang, rr, dtype)
    on = collide.bool()
    i, j = torch.meshgrid(torch.arange(O), torch.arange(O), indexing="ij")
    ok = (i != j) & (rr[i] == rr[j]) & on[i] & on[j]
    i, j = i[ok], j[ok]                                                                  # ordered pairs: row i against its partner j
    area = quad_intersection_area_torch(ring[:, i], ring[:, j])
    hov = torch.minimum(h1[:, i], h1[:, j]) - torch.maximum(h0[:, i], h0[:, j])
    live = hov > 0
    hov = torch.where(live, hov, torch.zeros_like(hov))
    area = torch.where(live, area, torch.zeros_like(area))
    penalty = torch.zeros(S, int(n_rooms), dtype=dtype)
    behind = j > i
    penalty.index_add_(1, rid[i[behind]], (area * hov)[:, behind])
    half = lambda x, y: torch.where(x < y, torch.ones_like(x), torch.where(x == y, torch.full_like(x, 0.5), torch.zeros_like(x)))
    g_h1 = torch.zeros(S, O, dtype=dtype).index_add_(1, i, area * half(h1[:, i], h1[:, j]))
    g_h0 = torch.zeros(S, O, dtype=dtype).index_add_(1, i, -area * half(h0[:, j], h0[:, i]))
    gv = torch.zeros(S, O, 4, 2, dtype=dtype).index_add_(1, i, quad_area_grad_torch(ring[:, i], ring[:, j]) * hov[..., None, None])
    # vertices and heights -> box[0:6], angle: vertex = R(theta) (+- half size) + centre, theta = -angle * float32(2 pi / 24)
    k24 = float(np.float32(2.0 * float(np.pi) / 24.0))
    ext = b[:, rr, 3:6]
    theta = -ang * k24
    c, s = torch.cos(theta)[..., None], torch.sin(theta)[..., None]
    hx, hz = (b[..., 3] * ext[..., 0] - b[..., 0] * ext[..., 0]) / 2, (b[..., 5] * ext[..., 2] - b[..., 2] * ext[..., 2]) / 2
    xs, zs = torch.stack([-hx, -hx, hx, hx], -1), torch.stack([-hz, hz, hz, -hz], -1)
    gx, gy = gv[..., 0], gv[..., 1]
    gxs, gzs = c * gx - s * gy, s * gx + c * gy
    gcx, gcz = gx.sum(-1), gy.sum(-1)
    gth = (gx * (-s * xs + c * zs) - gy * (c * xs + s * zs)).sum(-1)
    gmnx, gmxx, gmnz, gmxz = gxs[..., 0] + gxs[..., 1], gxs[..., 2] + gxs[..., 3], gzs[..., 0] + gzs[..., 3], gzs[..., 1] + gzs[..., 2]
    gb = torch.stack([ext[..., 0] * ((gmnx - gmxx + gcx) / 2), ext[..., 1] * g_h0, ext[..., 2] * ((gmnz - gmxz + gcz) / 2),
                      ext[..., 0] * ((gmxx - gmnx + gcx) / 2), ext[..., 1] * g_h1, ext[..., 2] * ((gmxz - gmnz + gcz) / 2)], -1)
    ga = -k24 * gth
    room_row = (rr == torch.arange(O))
    gb = torch.where(room_row[None, :, None], torch.zeros_like(gb), gb)
    ga = torch.where(room_row[None], torch.zeros_like(ga), ga)
    return penalty, gb, ga


# (the restatements of the --measure_acc_l1_std kernels)
def restore_boxes_torch(boxes, objs, room_cls):
    """restore_box (test_utils.py:119-132) of [S, O, 6] layouts, out of place"""
    S, O, _ = boxes.shape
    is_room = (objs == room_cls)
    nxt = torch.full((O,), -1, dtype=torch.int64)
    j = -1
    for i in range(O - 1, -1, -1):
        nxt[i] = j if not bool(is_room[i]) else -1
        if bool(is_room[i]):
            j = i
    out = boxes.clone()
    rows = torch.nonzero(nxt >= 0).flatten()
    if rows.numel():
        sc = boxes[:, nxt[rows], 3:6]
        out[:, rows, 0:3] = boxes[:, rows, 0:3] * sc
        out[:, rows, 3:6] = boxes[:, rows, 3:6] * sc
    return out


def compute_rel_torch(s, o):
    """compute_rel (utils.py:36-80) without the room branch for box pairs s, o [..., 6] float32 -> relation index, NONE (16) where
    the reference returns None.  The atan2 sector test is the comparison form of the device kernel (oracle/graph_build_ref.py)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    sx0, sy0, sz0, sx1, sy1, sz1 = s.unbind(-1)
    ox0, oy0, oz0, ox1, oy1, oz1 = o.unbind(-1)
    c1x, c1y, c1z = (sx0 + sx1) / 2, (sy0 + sy1) / 2, (sz0 + sz1) / 2
    c2y = (oy0 + oy1) / 2
    on = (c1x >= ox0) & (c1x <= ox1) & (c1z >= oz0) & (c1z <= oz1) & \
        (((c1y - c2y) - (sy1 - sy0 + oy1 - oy0) / 2).abs() < f(0.05))
    dx = c1x - (ox0 + ox1) / 2
    dz = c1z - (oz0 + oz1) / 2
    area_s = (sx1 - sx0) * (sz1 - sz0)
    area_o = (ox1 - ox0) * (oz1 - oz0)
    zero = torch.zeros_like(dx)
    area_i = torch.fmax(zero, torch.fmin(sx1, ox1) - torch.fmax(sx0, ox0)) * torch.fmax(zero, torch.fmin(sz1, oz1) - torch.fmax(sz0, oz0))
    iou = area_i / (area_s + area_o - area_i)
    touching = (f(0.0001) < iou) & (iou < f(0.5))
    t = lambda a, b: torch.where(touching, torch.full_like(dx, a, dtype=torch.int64), torch.full_like(dx, b, dtype=torch.int64))
    rel = t(_FRONT_T, _FRONT)
    rel = torch.where((dx > 0) & (-dx <= dz) & (dz < dx) | (dx == 0) & (dz == 0), t(_LEFT_T, _RIGHT), rel)
    rel = torch.where((dz < 0) & (dx.abs() < -dz), t(_BEHIND_T, _BEHIND), rel)
    rel = torch.where((dx < 0) & (dz.abs() <= -dx), t(_RIGHT_T, _LEFT), rel)
    rel = torch.where(torch.isnan(dx) | torch.isnan(dz), torch.full_like(rel, NONE), rel)
    rel = torch.where((sx0 > ox0) & (sx1 < ox1) & (sz0 > oz0) & (sz1 < oz1), torch.full_like(rel, _INSIDE), rel)
    rel = torch.where((sx0 < ox0) & (sx1 > ox1) & (sz0 < oz0) & (sz1 > oz1), torch.full_like(rel, _SURROUND), rel)
    return torch.where(on, torch.full_like(rel, _ON), rel)


def relation_acc_torch(boxes, objs, triples, room_cls, table):
    """relation_acc as torch ops: -> (good [S] int64, confusion [S, 16, 17] int64)"""
    S, O, _ = boxes.shape
    table = torch.as_tensor(table, dtype=torch.int64)
    triples = triples.to(torch.int64).reshape(-1, 3)
    ok = (triples[:, 0] >= 0) & (triples[:, 0] < O) & (triples[:, 2] >= 0) & (triples[:, 2] < O)
    tr = triples[ok]
    r = restore_boxes_torch(boxes.float(), objs, room_cls)
    rel = compute_rel_torch(r[:, tr[:, 0]], r[:, tr[:, 2]])                              # [S, T]
    rel = torch.where((objs[tr[:, 2]] == room_cls)[None], torch.full_like(rel, _IN_ROOM), rel)
    pg = tr[:, 1][None]
    hit = (rel < 16) & (table[rel.clamp(max=15)] >= 0) & (table[rel.clamp(max=15)] == pg)
    good = hit.sum(1)
    conf = torch.zeros(S, 16, 17, dtype=torch.int64)
    match = table[:, None] == tr[:, 1][None]                                             # [16, T]
    has = match.any(0) & (table[match.int().argmax(0)] >= 0)
    row = match.int().argmax(0)
    for s in range(S):
        idx = (row[has] * 17 + rel[s][has])
        conf[s].view(-1).scatter_add_(0, idx, torch.ones_like(idx))
    return good, conf


def layout_l1_torch(boxes, gt):
    """[S] float64: mean over O x 6 of the float32 |a - b| (accumulated in fp64)"""
    return (boxes.float() - gt.float()[None]).abs().double().flatten(1).sum(1) / (gt.shape[0] * 6)


def layout_spread_torch(boxes, angle_bins):
    """[3] float64: np.mean(np.std(., axis=0)) of the angle bins, centres and sizes (test_acc_mean_std.py:54-66)"""
    b = boxes.float()
    pos = b[..., :3] / 2.0 + b[..., 3:] / 2.0
    size = (b[..., :3] - b[..., 3:]).abs()
    std = lambda v: v.double().std(0, unbiased=False).mean()
    return torch.stack([std(angle_bins.double()), std(pos), std(size)])


def baselines_torch(gt, objs, room_cls, uniforms, normals):
    """[2, O, 6]: random_scene (test_utils.py:93-116) and boxes + float32(hstack([off, off])) (test_acc_mean_std.py:109-110)"""
    g = gt.float()
    u, n = uniforms.float(), normals.float()
    h = (g[:, 3:] - g[:, :3]) / 2
    rnd = torch.cat([u - h, u + h], 1)
    room = (objs == room_cls)[:, None]
    rnd = torch.where(room, g, rnd)
    per = g + torch.cat([n, n], 1)
    return torch.stack([rnd, per])


# ------------------------------------------------------------------------------------------------------------------------------
# the mode
# ------------------------------------------------------------------------------------------------------------------------------
def load_mean_cov(path):
    """the reference's stats file (testing/test_VAE.py:54-61: pickle of [mean_est, cov_est]) -> (mean [E], cov [E, E]) float64"""
    with open(path, "rb") as f:
        mean, cov = pickle.load(f)
    return torch.as_tensor(np.asarray(mean), dtype=torch.float64), torch.as_tensor(np.asarray(cov), dtype=torch.float64)


def save_mean_cov(path, mean, cov):
    """write (mean, cov) as the reference does: a pickled [mean_est, cov_est] of numpy arrays"""
    m = mean.detach().cpu().double().numpy() if torch.is_tensor(mean) else np.asarray(mean, np.float64)
    c = cov.detach().cpu().double().numpy() if torch.is_tensor(cov) else np.asarray(cov, np.float64)
    with open(path, "wb") as f:
        pickle.dump([m, c], f)


def _unpack(batch):
    """a collated batch: suncg_collate_fn's 8-tuple (ids, objs, boxes, triples, angles, attributes, obj_to_img, triple_to_img) or the
    5-tuple of sampling.posterior_stats (objs, triples, boxes, angles, attributes) -> (objs, triples, boxes, attributes)"""
    if len(batch) == 8:
        _, objs, boxes, triples, _, attributes, _, _ = batch
    elif len(batch) == 5:
        objs, triples, boxes, _, attributes = batch
    else:
        raise ValueError("a batch is suncg_collate_fn's 8-tuple or (objs, triples, boxes, angles, attributes)")
    return objs, triples, boxes, attributes


def _draw_z(model, objs, triples, attributes, n, mean, cov, gen):
    """z [n * O, E] ~ N(mean, cov) from the device generator ``gen`` (independent of the engine's Philox stream position)"""
    E, O = model.embedding_dim, objs.shape[0]
    eps = torch.randn(n * O, E, generator=gen, device=objs.device, dtype=torch.float32)
    L, mu = _S._factor(mean, cov, E, objs.device)
    z = torch.empty_like(eps)
    _lib.check(_lib.lib().sln_linear_forward(_lib.ptr(eps), eps.shape[0], E, _lib.ptr(L), _lib.ptr(mu), _lib.ptr(z), E, None, -1,
                                             _lib.current_stream_ptr()), "sln_linear_forward")
    return z


def measure_acc_l1_std(model, batches, mean, cov, vocab, n_std_samples=10, seed=None, draws=None, overlap=False):
    """testing/test_acc_mean_std.py: get_acc_l1 + get_std over ``batches`` (collated, on the model's device) -> the nine figures the
    reference prints: {'l1_pred', 'l1_rand', 'l1_pert', 'acc_pred', 'acc_rand', 'acc_pert', 'angle_std', 'position_std', 'size_std'}.

    Per batch: one decode (sampling.sample_layouts), one baselines launch, one relation launch over the three layouts, one L1 launch,
    ``n_std_samples`` decodes in one engine call and one spread launch; the figures accumulate on the device and are read back once.
    ``seed``: z and the baseline draws come from a device generator seeded with it (default: the engine's stream / torch's).
    ``draws``: per batch a dict {'z': [O, E], 'uniforms': [O, 3], 'normals': [O, 3], 'z_std': [n_std_samples, O, E]} replaces
    every draw (the reference's np.random draws can be replayed).
    ``overlap``: the dict gains 'overlap_pred' / 'overlap_rand' / 'overlap_pert' - the mean intersecting volume of a layout's
    furniture (``layout_overlap`` of the three layouts: the decoded angle bins, the ground-truth bins for the two baselines), one
    more launch per batch; it needs the batches' angles (the 8- or 5-tuple carries them)."""
    dev = next(model.parameters()).device
    room = room_class(vocab)
    table = relation_table(vocab)
    gen = None
    if seed is not None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
    good = torch.zeros(3, dtype=torch.int64, device=dev)
    l1 = torch.zeros(3, dtype=torch.float64, device=dev)
    spread = torch.zeros(3, dtype=torch.float64, device=dev)
    ov_vol = torch.zeros(3, dtype=torch.float64, device=dev) if overlap else None
    ov_pairs = torch.zeros(3, dtype=torch.int64, device=dev) if overlap else None
    names = list(vocab["object_idx_to_name"])
    n_batches, n_triples = 0, 0
    draws = list(draws) if draws is not None else None
    for bi, batch in enumerate(batches):
        objs, triples, boxes, attributes = _unpack(batch)
        O = objs.shape[0]
        if boxes.dim() != 2 or boxes.shape[1] != 6:
            raise ValueError("measure_acc_l1_std needs 3D boxes [O, 6]")
        d = draws[bi] if draws is not None else None
        # --- get_acc_l1: predicted, random, perturbed (test_acc_mean_std.py:104-118) ---
        if d is not None:
            z = d["z"].to(dev, torch.float32).reshape(O, -1)
        elif gen is not None:
            z = _draw_z(model, objs, triples, attributes, 1, mean, cov, gen)
        else:
            z = None
        bp, ap, _ = _S.sample_layouts(model, objs, triples, attributes, n_samples=1, mean=mean, cov=cov, z=z)
        lay = torch.empty(3, O, 6, dtype=torch.float32, device=dev)
        lay[0].copy_(bp[0])
        if d is not None:
            baselines(boxes, objs, room, uniforms=d["uniforms"].to(dev), normals=d["normals"].to(dev), out=lay[1:])
        else:
            key = torch.randint(-2 ** 62, 2 ** 62, (2,), dtype=torch.int64, device=dev, generator=gen)
            baselines(boxes, objs, room, key=key, out=lay[1:])
        relation_acc(lay, objs, triples, room, table, good=good)
        layout_l1(lay, boxes, out=l1)
        if overlap:
            gt_ang = (batch[4] if len(batch) == 8 else batch[3]).to(dev, torch.float32)
            ang = torch.stack([ap[0].to(torch.float32), gt_ang, gt_ang])
            layout_overlap(lay, ang, room_rows(objs, room), visible_rows(objs, names), vol=ov_vol, pairs=ov_pairs)
        # --- get_std (:39-69) ---
        if d is not None:
            z = d["z_std"].to(dev, torch.float32).reshape(n_std_samples * O, -1)
        elif gen is not None:
            z = _draw_z(model, objs, triples, attributes, n_std_samples, mean, cov, gen)
        else:
            z = None
        bs, ab, _ = _S.sample_layouts(model, objs, triples, attributes, n_samples=n_std_samples, mean=mean, cov=cov, z=z)
        layout_spread(bs, ab, out=spread)
        n_batches += 1
        n_triples += int(triples.shape[0])            # a host-side shape, no device read
    if n_batches == 0:
        raise ValueError("no batches")
    g, l, s = (t.cpu() for t in (good, l1, spread))   # the one read-back
    acc = [float(x) / n_triples if n_triples else float("nan") for x in g.tolist()]
    l = (l / n_batches).tolist()
    s = (s / n_batches).tolist()
    res = {"l1_pred": l[0], "l1_rand": l[1], "l1_pert": l[2], "acc_pred": acc[0], "acc_rand": acc[1], "acc_pert": acc[2],
           "angle_std": s[0], "position_std": s[1], "size_std": s[2]}
    if overlap:
        v = (ov_vol.cpu() / n_batches).tolist()
        res.update(overlap_pred=v[0], overlap_rand=v[1], overlap_pert=v[2])
    return res
