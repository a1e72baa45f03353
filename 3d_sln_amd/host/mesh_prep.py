"""Mesh preparation: split long edges before models enter the bank - the step ``models/misc.py:79,100`` takes with
``pymesh.split_long_edges_raw(V, F, 0.6)`` on every object model, wall sub-mesh, floor and ceiling.

The renderers drop a face whole when one corner lies behind the near plane (``diff_render.cull_and_classify``) and the pixel-map backward
walks pixels along face edges, so coarse meshes give holes and poor gradients.  pymesh is not available and its algorithm cannot be
pinned: the rule here is this project's own (DESIGN §4 "Splitting long edges"), stated exactly, and differs from pymesh in triangulation.

One pass over ``(v float32 [V,3], f int32 [F,3], origin [F])``:
  marking      edge k of a face joins corners k and (k+1) % 3; squared length ``(dx*dx + dy*dy) + dz*dz`` in float64 from the float32
               coordinates, no contraction; marked when it exceeds ``max_edge**2`` (float64, formed on the host);
  new vertices the marked edges of all faces keyed ``(min(i,j) << 32) | max(i,j)``; key rank u of the sorted unique keys becomes vertex
               ``V + u`` at ``float32((double(a) + double(b)) * 0.5)``; old vertices keep their indices;
  children     in this order, winding kept, m_k the midpoint of edge k:
                 0 marked   the face;
                 3 marked   (c0,m0,m2) (m0,c1,m1) (m2,m1,c2) (m0,m1,m2);
                 1 marked   edge k, A,B,C = c_k, c_k+1, c_k+2:  (A,m_k,C) (m_k,B,C);
                 2 marked   unmarked edge k, M1 = m_k+1, M2 = m_k+2:  (M2,M1,C), then the quad A,B,M1,M2 by its shorter diagonal
                            (squared float64 lengths of the float32 positions, a tie goes to A-M1):
                            |A M1|^2 <= |B M2|^2 ? (A,B,M1) (A,M1,M2) : (A,B,M2) (B,M1,M2);
  output       children in input face order at the exclusive prefix sum of the child counts, each with its parent's origin.
Passes repeat until none marks an edge.

``split_long_edges_np`` is the rule in numpy: the CPU route and what the kernels (``csrc/mesh_split.hip``: mark, midpoints, emit - three
launches per pass) are held to for equality.  Sorting the keys, the prefix sum and one read-back per pass are torch plumbing: this is
preparation, not a captured loop.
"""
import math

import numpy as np
import torch

from .. import _lib

_NEXT = (1, 2, 0)
STATUS_BAD_FACE = 1         # mark: a face with an index outside [0, V) - copied through unsplit
STATUS_BAD_KEY = 2          # midpoints: a key that names a vertex outside [0, V)
STATUS_BAD_EMIT = 4         # emit: an offset outside the output, or a new vertex index outside [V, V + U)


def _pass_bound(longest, max_edge):
    """every new edge is at most sqrt(3)/2 of its parent's longest (halves, midlines, medians): ceil(log(L / max_edge) / log(2 / sqrt 3))
    passes suffice; one more is allowed for the float32 rounding of the midpoints"""
    if not longest > max_edge:
        return 0
    return int(math.ceil(math.log(longest / max_edge) / math.log(2.0 / math.sqrt(3.0)))) + 1


def _too_many(total, max_faces):
    return ValueError("splitting would give %d faces, more than max_faces = %d: raise max_edge or max_faces" % (total, max_faces))


def _no_end(passes, max_edge):
    return RuntimeError("edges still longer than max_edge = %g after %d passes, the bound for this mesh: max_edge is below the float32 "
                        "spacing of the coordinates" % (max_edge, passes))


# ---------------------------------------------------------------- the rule in numpy
def _edge_sq_np(a, b):
    d = a - b                                                   # float64 [..., 3]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _pass_np(v, f, origin, thr, max_faces, passes, bound, max_edge):
    """-> None when no edge is marked, else (v_out, f_out, origin_out, unique keys, mask [F]); raises before anything of the output's
    size is formed"""
    V = v.shape[0]
    c = f.astype(np.int64)
    p = v.astype(np.float64)
    marked = np.stack([_edge_sq_np(p[c[:, k]], p[c[:, _NEXT[k]]]) > thr for k in range(3)], 1)          # [F, 3]
    if not marked.any():
        return None
    total = c.shape[0] + int(marked.sum())
    if total > max_faces:
        raise _too_many(total, max_faces)
    if passes >= bound:
        raise _no_end(passes, max_edge)
    nxt = c[:, list(_NEXT)]
    keys = np.where(marked, (np.minimum(c, nxt) << 32) | np.maximum(c, nxt), -1)
    ukeys, inv = np.unique(keys[marked], return_inverse=True)
    mid = np.full(c.shape, -1, dtype=np.int64)
    mid[marked] = V + inv.reshape(-1)
    v_new = ((p[ukeys >> 32] + p[ukeys & 0xFFFFFFFF]) * 0.5).astype(np.float32)
    v_out = np.concatenate([v, v_new])
    mask = marked[:, 0] * 1 + marked[:, 1] * 2 + marked[:, 2] * 4
    count = 1 + marked.sum(1)
    off = np.cumsum(count) - count
    f_out = np.empty((total, 3), dtype=np.int64)
    r = np.nonzero(mask == 0)[0]
    f_out[off[r]] = c[r]
    r = np.nonzero(mask == 7)[0]
    c0, c1, c2, m0, m1, m2 = c[r, 0], c[r, 1], c[r, 2], mid[r, 0], mid[r, 1], mid[r, 2]
    for j, tri in enumerate(((c0, m0, m2), (m0, c1, m1), (m2, m1, c2), (m0, m1, m2))):
        f_out[off[r] + j] = np.stack(tri, 1)
    q = v_out.astype(np.float64)
    for k in range(3):
        k1, k2 = _NEXT[k], _NEXT[_NEXT[k]]
        r = np.nonzero(mask == (1 << k))[0]                     # one marked: edge k
        A, B, Cc, M = c[r, k], c[r, k1], c[r, k2], mid[r, k]
        f_out[off[r]] = np.stack((A, M, Cc), 1)
        f_out[off[r] + 1] = np.stack((M, B, Cc), 1)
        r = np.nonzero(mask == (7 ^ (1 << k)))[0]               # two marked: edge k is not
        A, B, Cc, M1, M2 = c[r, k], c[r, k1], c[r, k2], mid[r, k1], mid[r, k2]
        first = _edge_sq_np(q[A], q[M1]) <= _edge_sq_np(q[B], q[M2])
        f_out[off[r]] = np.stack((M2, M1, Cc), 1)
        f_out[off[r] + 1] = np.where(first[:, None], np.stack((A, B, M1), 1), np.stack((A, B, M2), 1))
        f_out[off[r] + 2] = np.where(first[:, None], np.stack((A, M1, M2), 1), np.stack((B, M1, M2), 1))
    return v_out, f_out.astype(np.int32), np.repeat(origin, count), ukeys, mask


def _longest_np(v, f):
    p = v.astype(np.float64)
    c = f.astype(np.int64)
    return math.sqrt(max(float(_edge_sq_np(p[c[:, k]], p[c[:, _NEXT[k]]]).max()) for k in range(3)))


def _check_args(max_edge, max_faces):
    max_edge = float(max_edge)
    if not (math.isfinite(max_edge) and max_edge > 0.0):
        raise ValueError("max_edge must be a positive finite length, got %r" % (max_edge,))
    return max_edge, int(max_faces)


def _run_np(v, f, max_edge, max_faces, face_mesh=None, n_mesh=1, owner=None):
    """the pass loop on the host -> (v, f, origin, per-mesh pass counts, longest input edge, vertex owner or None)"""
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(f).astype(np.int32).reshape(-1, 3))
    if v.shape[0] < 1 or f.shape[0] < 1:
        raise ValueError("an empty mesh cannot be split")
    if not np.isfinite(v).all():
        raise ValueError("vertices are not finite")
    if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
        raise IndexError("faces index vertices outside [0, %d)" % v.shape[0])
    if v.shape[0] + 3 * f.shape[0] >= 2 ** 31:
        raise ValueError("V + 3 F must stay below 2^31")
    thr = float(max_edge) * float(max_edge)
    origin = np.arange(f.shape[0], dtype=np.int32)
    per_mesh = np.zeros(n_mesh, dtype=np.int64)
    face_mesh = np.zeros(f.shape[0], dtype=np.int64) if face_mesh is None else face_mesh
    longest = _longest_np(v, f)
    bound, passes = _pass_bound(longest, max_edge), 0
    while True:
        res = _pass_np(v, f, origin, thr, max_faces, passes, bound, max_edge)
        if res is None:
            break
        per_mesh[np.unique(face_mesh[origin[res[4] > 0]])] += 1
        if owner is not None:
            owner = np.concatenate([owner, owner[res[3] >> 32]])
        v, f, origin = res[:3]
        passes += 1
    return v, f, origin, per_mesh, longest, owner


def split_long_edges_np(v, f, max_edge=0.6, max_faces=1 << 22):
    """The rule in numpy (no kernel code involved): ``v`` [V, 3], ``f`` [F, 3] arrays -> ``(v_out float32, f_out int32, info)`` with
    ``info = dict(origin int32 [F_out], passes, status = 0, longest_in)``."""
    max_edge, max_faces = _check_args(max_edge, max_faces)
    v, f, origin, per_mesh, longest, _ = _run_np(v, f, max_edge, max_faces)
    return v, f, dict(origin=origin, passes=int(per_mesh[0]), status=0, longest_in=longest)


# ---------------------------------------------------------------- the kernels
def _edge_sq_t(p, c, k):
    d = p[c[:, k]] - p[c[:, _NEXT[k]]]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _run_device(v, f, max_edge, max_faces, face_mesh=None, n_mesh=1, owner=None, validate=True):
    """the pass loop on the device: per pass three launches of csrc/mesh_split.hip, torch's sort / unique and cumsum between them and
    one read-back (the child total and whether a key is unmarked); one read-back before the loop (the checks, the longest edge) and
    one behind it -> (v, f, origin, per-mesh passes, per-mesh longest input edge, vertex owner or None, status)"""
    L, P, st = _lib.lib(), _lib.ptr, _lib.current_stream_ptr
    dev = v.device
    v = v.detach().to(torch.float32).reshape(-1, 3).contiguous()
    f = f.detach().to(torch.int32).reshape(-1, 3).contiguous()
    V, F = int(v.shape[0]), int(f.shape[0])
    if V < 1 or F < 1:
        raise ValueError("an empty mesh cannot be split")
    if V + 3 * F >= 2 ** 31:
        raise ValueError("V + 3 F must stay below 2^31")
    thr = float(max_edge) * float(max_edge)
    face_mesh = torch.zeros(F, dtype=torch.int64, device=dev) if face_mesh is None else face_mesh
    good = ((f >= 0) & (f < V)).all(1)
    c, p = f.long().clamp(0, V - 1), v.double()
    sq = torch.stack([_edge_sq_t(p, c, k) for k in range(3)]).max(0).values
    sq = torch.where(good, sq, torch.zeros_like(sq)).nan_to_num(nan=0.0)                       # (a face outside the table has no edges)
    mesh_sq = torch.zeros(n_mesh, dtype=torch.float64, device=dev).scatter_reduce_(0, face_mesh, sq, "amax")
    finite, all_good, longest = torch.stack([torch.isfinite(v).all().double(), good.all().double(), sq.max()]).tolist()
    if not finite:
        raise ValueError("vertices are not finite")
    if validate and not all_good:
        raise IndexError("faces index vertices outside [0, %d)" % V)
    longest = math.sqrt(longest)
    # a face outside the table stays outside in every pass: an index >= V would name a NEW vertex after the first one, so the loop
    # runs with (-1, -1, -1) in its place (the kernels copy it through and flag it) and the face's own indices come back at the end
    bad_rows = saved = None
    if not all_good:
        bad_rows = torch.nonzero(~good).reshape(-1)
        saved = f[bad_rows].clone()
        f = f.clone()
        f[bad_rows] = -1
    del c, p, sq, good
    bound, passes = _pass_bound(longest, max_edge), 0
    origin = torch.arange(F, dtype=torch.int32, device=dev)
    per_mesh = torch.zeros(n_mesh, dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    while True:
        V, F = int(v.shape[0]), int(f.shape[0])
        mask = torch.empty(F, dtype=torch.int32, device=dev)
        count = torch.empty(F, dtype=torch.int32, device=dev)
        keys = torch.empty(F, 3, dtype=torch.int64, device=dev)
        _lib.check(L.sln_mesh_split_mark(P(v), V, P(f), F, thr, P(mask), P(count), P(keys), P(status), st()), "sln_mesh_split_mark")
        ukeys, inv = torch.unique(keys.reshape(-1), sorted=True, return_inverse=True)          # -1 (unmarked) sorts first
        cum = torch.cumsum(count, 0)
        total, skip = (int(x) for x in torch.stack([cum[-1], (ukeys[0] < 0).long()]).tolist())
        if total > max_faces:
            raise _too_many(total, max_faces)
        if total == F:
            break
        if passes >= bound:
            raise _no_end(passes, max_edge)
        ukeys = ukeys[skip:].contiguous()
        U = int(ukeys.numel())
        mid = (inv.reshape(F, 3) + (V - skip)).to(torch.int32)
        mid = torch.where(keys >= 0, mid, torch.full_like(mid, -1)).contiguous()
        offsets = (cum - count).contiguous()                                                    # int64, exclusive
        v_out = torch.empty(V + U, 3, dtype=torch.float32, device=dev)
        v_out[:V] = v
        _lib.check(L.sln_mesh_split_midpoints(P(v), V, P(ukeys), U, P(v_out[V:]), P(status), st()), "sln_mesh_split_midpoints")
        f_out = torch.empty(total, 3, dtype=torch.int32, device=dev)
        origin_out = torch.empty(total, dtype=torch.int32, device=dev)
        _lib.check(L.sln_mesh_split_emit(P(v_out), V, U, P(f), P(origin), P(mask), P(offsets), P(mid), F, total, P(f_out), P(origin_out),
                                         P(status), st()), "sln_mesh_split_emit")
        hit = torch.zeros(n_mesh, dtype=torch.int64, device=dev).index_add_(0, face_mesh[origin.long()], (mask > 0).long())
        per_mesh += (hit > 0).long()
        if owner is not None:
            owner = torch.cat([owner, owner[ukeys >> 32]])
        v, f, origin = v_out, f_out, origin_out
        passes += 1
    if bad_rows is not None:
        rows = torch.nonzero(torch.isin(origin, bad_rows.to(torch.int32))).reshape(-1)
        f = f.clone()
        f[rows] = saved[torch.searchsorted(bad_rows, origin[rows].long())]
    tail = torch.cat([per_mesh.double(), mesh_sq, status.sum().double().reshape(1)]).tolist()
    return v, f, origin, [int(x) for x in tail[:n_mesh]], [math.sqrt(x) for x in tail[n_mesh:2 * n_mesh]], owner, int(tail[-1])


def split_long_edges(v, f, max_edge=0.6, max_faces=1 << 22, validate=True):
    """``pymesh.split_long_edges_raw``'s call shape: ``(v [V,3], f [F,3], max_edge)`` -> ``(v_out float32, f_out int32, info)``,
    ``info = dict(origin, passes, status, longest_in)``: the input face of every output face, the passes that split something, the
    kernels' status bits (0 on the host route) and the longest input edge.  Device tensors take the kernels (a missing library is an
    error), host tensors and arrays take ``split_long_edges_np`` (tensors in, tensors out).  ValueError: non-finite vertices, a
    max_edge that is not positive and finite, more than ``max_faces`` faces after a pass (raised before that pass allocates);
    IndexError: faces outside the vertex table.  ``validate=False`` (device route only) skips that last check: such a face comes
    through unsplit, in every pass, and sets ``STATUS_BAD_FACE`` in ``info['status']``."""
    max_edge, max_faces = _check_args(max_edge, max_faces)
    if isinstance(v, torch.Tensor) and v.is_cuda:
        f = torch.as_tensor(f, device=v.device) if not isinstance(f, torch.Tensor) else f.to(v.device)
        v, f, origin, per_mesh, longest, _, status = _run_device(v, f, max_edge, max_faces, validate=validate)
        return v, f, dict(origin=origin, passes=per_mesh[0], status=status, longest_in=longest[0])
    as_tensor = isinstance(v, torch.Tensor)
    vn = v.detach().cpu().numpy() if as_tensor else v
    fn = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f
    v, f, info = split_long_edges_np(vn, fn, max_edge, max_faces)
    if as_tensor:
        v, f, info["origin"] = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(info["origin"])
    return v, f, info


def split_meshes(meshes, max_edge=0.6, max_faces=1 << 22):
    """``meshes``: a list of ``(v, f)`` pairs, all device tensors or all host tensors / arrays -> a list of ``(v_out, f_out, info)``, each
    equal to the mesh's own ``split_long_edges`` result.  The meshes are split as ONE concatenated mesh (one launch sequence per pass
    serves them all) and separated again by stable compaction: the vertex offsets are monotone per mesh, so key order, and with it every
    new vertex index, is the mesh's own; a mesh's vertices come out as its originals, then each pass's new vertices in key order.  A
    mesh without faces is returned as it came.  ``max_faces`` bounds the concatenated mesh."""
    max_edge, max_faces = _check_args(max_edge, max_faces)
    meshes = list(meshes)
    if not meshes:
        return []
    on_dev = isinstance(meshes[0][0], torch.Tensor) and meshes[0][0].is_cuda
    as_tensor = [isinstance(m[0], torch.Tensor) for m in meshes]
    if on_dev:
        dev = meshes[0][0].device
        vs = [m[0].detach().to(device=dev, dtype=torch.float32).reshape(-1, 3) for m in meshes]
        fs = [torch.as_tensor(m[1]).to(device=dev, dtype=torch.int32).reshape(-1, 3) for m in meshes]
    else:
        vs = [np.asarray(m[0].detach().cpu().numpy() if isinstance(m[0], torch.Tensor) else m[0], dtype=np.float32).reshape(-1, 3) for m in meshes]
        fs = [np.asarray(m[1].detach().cpu().numpy() if isinstance(m[1], torch.Tensor) else m[1]).astype(np.int32).reshape(-1, 3) for m in meshes]
    live = [k for k in range(len(meshes)) if fs[k].shape[0] > 0 and vs[k].shape[0] > 0]
    out = [None] * len(meshes)
    for k in range(len(meshes)):
        if k not in live:
            z = torch.zeros(0, dtype=torch.int32, device=vs[k].device) if on_dev else np.zeros(0, dtype=np.int32)
            out[k] = (vs[k], fs[k], dict(origin=z, passes=0, status=0, longest_in=0.0))
    if not live:
        return out
    nv, nf = [int(vs[k].shape[0]) for k in live], [int(fs[k].shape[0]) for k in live]
    voff, foff = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(nf)])
    ids = np.arange(len(live), dtype=np.int64)
    if on_dev:
        # whole-bank tensor expressions, three read-backs besides the pass loop's: a loop over the meshes would cost more than the split
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        n = len(live)
        fm_in, f = T(np.repeat(ids, nf)), torch.cat([fs[k] for k in live])
        inside = ((f >= 0) & (f < T(np.repeat(nv, nf).astype(np.int32))[:, None])).all(1)
        if not bool(inside.all()):
            k = live[int(fm_in[torch.nonzero(~inside)[0, 0]])]
            raise IndexError("faces of mesh %d index vertices outside [0, %d)" % (k, vs[k].shape[0]))
        f = f + T(np.repeat(voff[:-1], nf).astype(np.int32))[:, None]
        v, f, origin, per_mesh, longest, owner, status = _run_device(torch.cat([vs[k] for k in live]), f, max_edge, max_faces, fm_in, n,
                                                                     T(np.repeat(ids, nv)))
        order = torch.argsort(owner, stable=True)                    # a mesh's originals, then each pass's new vertices in key order
        vcount = torch.bincount(owner, minlength=n)
        local = torch.empty(v.shape[0], dtype=torch.int32, device=dev)
        local[order] = (torch.arange(v.shape[0], device=dev) - (torch.cumsum(vcount, 0) - vcount)[owner[order]]).to(torch.int32)
        face_mesh = fm_in[origin.long()]                              # non-decreasing: a mesh's faces are one slice
        fcount = torch.bincount(face_mesh, minlength=n)
        counts = torch.cat([vcount, fcount]).tolist()
        v_parts = torch.split(v[order], counts[:n])
        f_parts = torch.split(local[f.long()], counts[n:])
        o_parts = torch.split(origin - T(foff[:-1].astype(np.int32))[face_mesh], counts[n:])
        for j, k in enumerate(live):
            out[k] = (v_parts[j], f_parts[j], dict(origin=o_parts[j], passes=per_mesh[j], status=status, longest_in=longest[j]))
        return out
    for k in live:
        lo, hi = int(fs[k].min()), int(fs[k].max())
        if lo < 0 or hi >= vs[k].shape[0]:
            raise IndexError("faces of mesh %d index vertices outside [0, %d)" % (k, vs[k].shape[0]))
    v = np.concatenate([vs[k] for k in live])
    f = np.concatenate([fs[k] + np.int32(voff[j]) for j, k in enumerate(live)])
    v, f, origin, per_mesh, _, owner = _run_np(v, f, max_edge, max_faces, np.repeat(ids, nf), len(live), np.repeat(ids, nv))
    face_mesh = np.repeat(ids, nf)[origin]
    for j, k in enumerate(live):
        mine = np.nonzero(owner == j)[0]
        local = np.zeros(v.shape[0], dtype=np.int32)
        local[mine] = np.arange(mine.size, dtype=np.int32)
        rows = np.nonzero(face_mesh == j)[0]
        vo, fo, oo = v[mine], local[f[rows]], (origin[rows] - np.int32(foff[j])).astype(np.int32)
        if as_tensor[k]:
            vo, fo, oo = torch.from_numpy(vo), torch.from_numpy(fo), torch.from_numpy(oo)
        out[k] = (vo, fo, dict(origin=oo, passes=int(per_mesh[j]), status=0, longest_in=_longest_np(vs[k], fs[k])))
    return out
