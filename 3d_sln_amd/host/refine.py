"""Layout refinement on the MI355X: counterpart of ``testing/test_render_refine.py::finetune_VAE`` (:243-359)
and of the scene assembly inside ``models/diff_render.py::mesh_render_func`` (:48-342).

What is reproduced from the reference
  * object placement (diff_render.py:76-159): box -> centre/size in room units, ``theta = -angle * 2pi/24``,
    isotropic scale ``min(size / model_size)``, rotation about y, translation ``centre - scale * R @ model_centre``;
    non-furniture classes are skipped (:93-97); the size loss (:98-100,160-165);
  * the room box of the last row is frozen to the first iteration's value (:55-60);
  * ``softargmax`` (test_render_refine.py:20-25), the ``fix_grad`` / ``quad_grad`` hooks (:217-228), the null-fill,
    ``PSP_pool_new`` multi-scale pooling (:192-215), ``loss = 100*0.5*L1(depth) + 100*sum CE/800 + 2*size_loss``
    and the per-iteration ``SGD(lr=2e-4, momentum=0.1, nesterov)`` over ``z`` (model parameters at lr/10) (:286-359).
What is replaced
  * mesh loading (models/misc.py: SUNCG meshes + pywavefront + pymesh, out of scope): without caller-supplied meshes every object
    class gets a procedural cuboid "model" with a fixed aspect ratio and walls / floor / ceiling are quads built from the room box;
    meshes stay resident on the GPU instead of being re-read from disk every iteration (models/misc.py:111-121).  The retrieval
    AMONG a class's models (models/misc.py:34-64,123-152) is reproduced: ``retrieve_choice`` / host/retrieve.py; so is the splitting
    of long edges (:79,100), by a rule of this project's own: ``MeshBank.from_arrays(max_edge=)`` / host/mesh_prep.py;
  * the 33 raster passes per call: one fused HIP pass (diff_render.scene_render semantics).
``render_fn`` is injectable so that the tests can run the very same loss graph on the CPU oracle.
"""
import collections
import copy
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import diff_render as DR
from . import evaluate as EV
from . import mesh_prep as MP
from . import observe as OB
from . import reproject as RP
from . import retrieve as RT
from . import scene_pictures as SP
from . import synthetic
from .sampling import _precision
from .. import _lib

DO_NOT_VIS = ["wall", "ceiling", "floor", "person", "door", "window", "curtain", "blinds"]


def softargmax(input_vec, sum_dim, beta=2.0):
    idx = torch.cumsum(torch.ones_like(input_vec), dim=sum_dim)
    return torch.sum(F.softmax(input_vec * beta, dim=sum_dim) * idx, dim=sum_dim) - 1.0


def fix_grad(g):
    avg = g[:, 3:] / 2.0 + g[:, :3] / 2.0
    return torch.cat([avg, avg], dim=1)


def quad_grad(g):
    return g * 4.0


def psp_pool(feats, sizes=(32, 48, 64, 96), as_list=False):
    """PSP_pool_new: bilinear(align_corners=True) to each size, then bilinear (default) to the largest."""
    outs = [F.interpolate(F.interpolate(feats, size=(s, s), mode='bilinear', align_corners=True), size=(sizes[-1], sizes[-1]),
                          mode='bilinear', align_corners=False) for s in sizes]
    return outs if as_list else torch.cat(outs, 1)


class MeshBank:
    """The model table, resident on the device.  Built plainly: a procedural stand-in, one cuboid model per class; ``from_arrays``: the
    caller's meshes, one or many per class (``models[name]`` is a class's model 0, ``model_list(name)`` all of them)."""

    def __init__(self, class_names, device, subdiv=2, seed=0):
        rng = np.random.default_rng(seed)
        self.models = {}
        for name in class_names:
            size = rng.uniform(0.5, 1.5, size=3)
            v, f = synthetic._grid_cuboid(-size / 2 + rng.uniform(-0.1, 0.1, size=3), size / 2, subdiv)
            v = torch.from_numpy(v.astype(np.float32)).to(device)
            self.models[name] = dict(v=v, f=torch.from_numpy(f.astype(np.int32)).to(device),
                                     bbox_min=v.min(0).values, bbox_max=v.max(0).values)


    vocab = None        # class list of the scene tensor's planes (object_idx_to_name[1:], diff_render.py:65); None: synthetic.FURNITURE
    shell = None        # wall / floor / ceiling meshes + their table boxes (see from_arrays); None: quads built from the room box
    shells = None       # every shell the caller listed (shell is entry 0)

    @classmethod
    def from_arrays(cls, meshes, device, vocab=None, shell=None, max_edge=None):
        """Caller-supplied meshes - the seam of models/diff_render.py:62,131, where the reference hands the retrieved SUNCG model's
        vertices / faces to the placement: ``meshes`` = {class name: (V [n,3] float, F [m,3] int)} or (V, F, bbox_min, bbox_max)
        (one model per class, any topology; faces index V), or a LIST of such models per class, each (V, F, bbox_min, bbox_max[, id])
        or a dict with those keys (``v, f, bbox_min, bbox_max, id``) - the class's rows of suncg_data_many.json, among which
        ``retrieve.retrieve_models`` picks per object (models/misc.py:34-64); ids default to ``"<class>#<k>"`` and are unique within a
        class.  The bounding box the placement scales by is the model table's (diff_render.py:106-115 read ``bbox_min`` / ``bbox_max`` of
        suncg_data) - the vertices' own when none is given.
        ``vocab``: the class list that lays out the 70 planes (``object_idx_to_name[1:]``, diff_render.py:65-69,372-379).
        ``shell``: the room's retrieved wall / floor / ceiling (diff_render.py:166-342) as arrays - dict(wall_v [n,3], wall_f = list of
        [m,3] sub-meshes over wall_v (models/misc.py:84-104), wall_bbox [2,3], floor_v, floor_f, floor_bbox [2,3], ceil_v, ceil_f), or a
        LIST of such dicts (the rows of wall_data_wfc.json, among which ``retrieve.retrieve_shell`` picks per room; entry 0 is the
        default); without it the shell is five quads on the room box.
        ``bank.table`` is the ``retrieve.ModelTable`` of the models, ``bank.shell_ratios`` the shell list's ratio tables.
        ``max_edge``: split every edge longer than this (models/misc.py:79,100 pass 0.6 to pymesh.split_long_edges_raw) - one
        ``mesh_prep.split_meshes`` call over every model of every class and every shell's wall, floor and ceiling, on ``device``.  A
        wall is split as one mesh over ``wall_v`` and its sub-meshes keep their faces' children.  Boxes, ids and the retrieval table
        stay those of the input (a midpoint never leaves the hull).  None: the meshes enter as they are."""
        bank = cls.__new__(cls)
        bank.models, bank.model_lists = {}, {}
        for name, mesh in meshes.items():
            many = isinstance(mesh, list) and len(mesh) > 0 and all(isinstance(m, (tuple, dict)) for m in mesh)
            entries, seen = [], set()
            for k, one in enumerate(mesh if many else [mesh]):
                if isinstance(one, dict):
                    one = (one["v"], one["f"], one.get("bbox_min"), one.get("bbox_max"), one.get("id"))
                one = tuple(one) + (None,) * (5 - len(one))
                V, F, blo, bhi, mid = one[:5]
                v = torch.as_tensor(np.asarray(V, dtype=np.float32)).reshape(-1, 3).to(device)
                f = torch.as_tensor(np.asarray(F).astype(np.int32)).reshape(-1, 3).to(device)
                if v.shape[0] == 0 or f.shape[0] == 0:
                    raise ValueError("mesh of class %r is empty" % (name,))
                if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
                    raise IndexError("faces of class %r index vertices outside [0, %d)" % (name, v.shape[0]))
                lo = torch.as_tensor(np.asarray(blo, dtype=np.float32)).to(device) if blo is not None else v.min(0).values
                hi = torch.as_tensor(np.asarray(bhi, dtype=np.float32)).to(device) if bhi is not None else v.max(0).values
                mid = str(mid) if mid is not None else "%s#%d" % (name, k)
                if mid in seen:
                    raise ValueError("class %r lists the model id %r twice" % (name, mid))
                seen.add(mid)
                # the table's own numbers (float64, as json gives them) for the retrieval's ratios
                lo64 = np.asarray(blo, dtype=np.float64) if blo is not None else lo.double().cpu().numpy()
                hi64 = np.asarray(bhi, dtype=np.float64) if bhi is not None else hi.double().cpu().numpy()
                entries.append(dict(v=v.contiguous(), f=f.contiguous(), bbox_min=lo, bbox_max=hi, id=mid, lo64=lo64, hi64=hi64))
            bank.models[name] = entries[0]
            bank.model_lists[name] = entries
        bank.vocab = list(vocab) if vocab is not None else None
        if shell is not None:
            bank.shells = [cls._shell_arrays(sh) for sh in (shell if isinstance(shell, list) else [shell])]
            if not bank.shells:
                raise ValueError("shell is an empty list")
            bank.shell = bank.shells[0]
        if max_edge is not None:
            cls._split_long_edges(bank, torch.device(device), max_edge)
        return bank

    @staticmethod
    def _split_long_edges(bank, dev, max_edge):
        entries = [e for lst in bank.model_lists.values() for e in lst]
        jobs = [(e["v"], e["f"]) for e in entries]
        shells = getattr(bank, "shells", None) or []
        for sh in shells:
            wall_f = np.concatenate(sh["wall_f"]) if sh["wall_f"] else np.zeros((0, 3), dtype=np.int64)
            for v, f in ((sh["wall_v"], wall_f), (sh["floor_v"], sh["floor_f"]), (sh["ceil_v"], sh["ceil_f"])):
                jobs.append((torch.from_numpy(np.ascontiguousarray(v.reshape(-1, 3))).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev)))
        res = MP.split_meshes(jobs, max_edge)
        for e, (v, f, _) in zip(entries, res):
            e["v"], e["f"] = v.clone(), f.clone()                 # (their own storage: the results are slices of the bank-wide tables)
        at = len(entries)
        for sh in shells:
            (wv, wf, winfo), (fv, ff, _), (cv, cf, _) = res[at:at + 3]
            at += 3
            origin, wf = winfo["origin"].cpu().numpy(), wf.cpu().numpy().astype(np.int64)
            ends = np.cumsum([0] + [f.shape[0] for f in sh["wall_f"]])
            sh["wall_f"] = [wf[(origin >= a) & (origin < b)] for a, b in zip(ends[:-1], ends[1:])]
            sh["wall_v"], sh["floor_v"], sh["ceil_v"] = (x.cpu().numpy() for x in (wv, fv, cv))
            sh["floor_f"], sh["ceil_f"] = ff.cpu().numpy().astype(np.int64), cf.cpu().numpy().astype(np.int64)

    @staticmethod
    def _shell_arrays(shell):
        sh = {k: (np.asarray(shell[k], dtype=np.float32) if not k.endswith("_f") else None) for k in shell}
        sh["wall_f"] = [np.asarray(f).astype(np.int64).reshape(-1, 3) for f in shell["wall_f"]]
        sh["floor_f"], sh["ceil_f"] = (np.asarray(shell[k]).astype(np.int64).reshape(-1, 3) for k in ("floor_f", "ceil_f"))
        for f, nv, what in [(f, sh["wall_v"].shape[0], "wall") for f in sh["wall_f"]] + [(sh["floor_f"], sh["floor_v"].shape[0], "floor"),
                                                                                            (sh["ceil_f"], sh["ceil_v"].shape[0], "ceiling")]:
            if f.size and (int(f.min()) < 0 or int(f.max()) >= nv):
                raise IndexError("faces of the %s index vertices outside [0, %d)" % (what, nv))
        sh["wall_bbox64"], sh["floor_bbox64"] = np.asarray(shell["wall_bbox"], dtype=np.float64), np.asarray(shell["floor_bbox"], dtype=np.float64)
        return sh

    def model_list(self, name):
        """the models of a class in table order (a bank of one model per class: that model)"""
        lists = getattr(self, "model_lists", None)
        return [self.models[name]] + (lists[name][1:] if lists and name in lists else [])

    def table_vocab(self):
        """``object_idx_to_name`` as the model table indexes it: '__room__', the planes' classes, then any further class with a model"""
        names = ["__room__"] + _classes_of(self)
        return names + sorted(n for n in self.models if n not in names)

    @property
    def table(self):
        """the ``retrieve.ModelTable`` of this bank's models, on the models' device (built on first use)"""
        t = self.__dict__.get("_table")
        if t is None:
            data, dev = {}, "cpu"
            for name in self.models:
                entries = self.model_list(name)
                dev = entries[0]["v"].device
                data[name] = [dict(id=e.get("id", "%s#%d" % (name, k)), bbox_min=e.get("lo64", e["bbox_min"].double().cpu().numpy()),
                                   bbox_max=e.get("hi64", e["bbox_max"].double().cpu().numpy())) for k, e in enumerate(entries)]
            t = self.__dict__["_table"] = RT.ModelTable(data, self.table_vocab(), dev)
        return t

    @property
    def shell_ratios(self):
        """(wall_ratio [W, 2], floor_ratio [W]) float64 host tensors of the shell list; None for the procedural shell"""
        shells = getattr(self, "shells", None)
        if not shells:
            return None
        r = self.__dict__.get("_shell_ratios")
        if r is None:
            rows = [dict(wall_bbox_min=sh["wall_bbox64"][0], wall_bbox_max=sh["wall_bbox64"][1], floor_bbox_min=sh["floor_bbox64"][0],
                         floor_bbox_max=sh["floor_bbox64"][1]) for sh in shells]
            r = self.__dict__["_shell_ratios"] = tuple(torch.from_numpy(x) for x in RT.shell_ratios(rows))
        return r

    def has_choice(self):
        """is there anything to retrieve: a class with more than one model, or more than one shell"""
        return any(len(v) > 1 for v in getattr(self, "model_lists", {}).values()) or len(getattr(self, "shells", None) or ()) > 1


def _classes_of(bank):
    return list(bank.vocab) if getattr(bank, "vocab", None) is not None else list(synthetic.FURNITURE)


_PROCEDURAL_SHELL = ("floor", "ceiling", "wall", "wall", "wall")
_SHELL_DIV = 6


def _shell_of(bank, shell=None):
    """the arrays of the chosen shell: ``shell`` = (wall entry, floor entry) of the bank's shell list (None, or an index < 0: entry 0).
    The ceiling follows the wall entry, as load_ceil_obj(wall_data) does (diff_render.py:285)."""
    sh = getattr(bank, "shell", None)
    if sh is None or shell is None:
        return sh
    shells = getattr(bank, "shells", None) or [sh]
    w, f = (shells[int(k)] if int(k) >= 0 else shells[0] for k in shell)
    if w is f:
        return w
    out = dict(w)
    out.update(floor_v=f["floor_v"], floor_f=f["floor_f"], floor_bbox=f["floor_bbox"])
    return out


def shell_topology(bank, shell=None):
    """[(class, vertex count, faces [m,3] int64 numpy)] of the room shell in buffer order - does not depend on the room."""
    sh = _shell_of(bank, shell)
    if sh is None:
        unit = np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
        v, f = synthetic._grid_quad(unit[0], unit[1], unit[2], _SHELL_DIV)
        return [(nm, v.shape[0], f.astype(np.int64)) for nm in _PROCEDURAL_SHELL]
    # reference order (diff_render.py:166-342): every wall sub-mesh with its own copy of the wall's vertices, the floor, the ceiling
    return ([("wall", sh["wall_v"].shape[0], f) for f in sh["wall_f"]] +
            [("floor", sh["floor_v"].shape[0], sh["floor_f"]), ("ceiling", sh["ceil_v"].shape[0], sh["ceil_f"])])


def _scaled_into_room(v, scale, model_center, center):
    """diff_render.py:188-200: [I | center - scale * model_center] x diag(scale) as two 4x4 matrices applied to the homogeneous
    vertices - in fp32 on the host with the reference's operation order, so that the shell's vertices are the reference's bit for bit"""
    move, grow = torch.eye(4), torch.eye(4)
    move[:3, 3] = center - scale * model_center
    grow[:3, :3] = grow[:3, :3] * scale
    hom = torch.cat((v.t(), torch.ones(1, v.shape[0])), 0)
    return torch.matmul(torch.matmul(move, grow)[:3], hom).t().contiguous()


def place_shell(bank, room_ext, shell=None):
    """Vertices of the room shell in room coordinates, [sum of shell_topology's vertex counts, 3] fp32 on the host.  ``shell``: the
    chosen (wall, floor) entries of the bank's shell list (``retrieve.retrieve_shell``; None: entry 0) - the ceiling is the wall entry's.
    Procedural bank: floor, ceiling, back / left / right wall on the room box.  Bank with shell tables: diff_render.py:166-342 - the
    walls are scaled isotropically by the LARGEST ratio of room extent to the table's wall box and centred in the room, a wall
    sub-mesh that comes closer to the camera than 0.9 of the depth while its mean x lies in the middle 80 % of the width is dropped
    (:203-213; here: its vertices collapse to one point, so that the face list keeps its shape and order); floor: x / z ratios, y = 0;
    ceiling: x / z ratios of its own bounding box, resting on the room's height.  One-off per room: the room row is frozen (:55-60)."""
    sh = _shell_of(bank, shell)
    room = [float(x) for x in room_ext]
    if sh is None:
        quads = [((0, 0, 0), (0, 0, room[2]), (room[0], 0, 0)), ((0, room[1], 0), (room[0], 0, 0), (0, 0, room[2])),
                 ((0, 0, 0), (room[0], 0, 0), (0, room[1], 0)), ((0, 0, 0), (0, room[1], 0), (0, 0, room[2])),
                 ((room[0], 0, 0), (0, 0, room[2]), (0, room[1], 0))]               # floor, ceiling, three walls (the order of shell_topology)
        sv = [synthetic._grid_quad(np.array(p0, np.float64), np.array(du, np.float64), np.array(dv, np.float64), _SHELL_DIV)[0] for p0, du, dv in quads]
        return torch.from_numpy(np.concatenate(sv).astype(np.float32))
    ext = torch.tensor(room, dtype=torch.float32)
    T = torch.from_numpy
    lo, hi = T(sh["wall_bbox"][0]), T(sh["wall_bbox"][1])
    wall = _scaled_into_room(T(sh["wall_v"]), torch.max(ext / (hi - lo)), (lo + hi) / 2.0, ext / 2.0)
    parts = []
    for f in sh["wall_f"]:
        fz, fx = wall[:, 2][T(f)], wall[:, 0][T(f)]
        drop = f.shape[0] > 0 and bool(fz.max() > 0.9 * ext[2]) and bool(fx.mean() > 0.1 * ext[0]) and bool(fx.mean() < 0.9 * ext[0])
        parts.append(torch.zeros_like(wall) if drop else wall)
    lo, hi = T(sh["floor_bbox"][0]), T(sh["floor_bbox"][1])
    span = hi - lo
    parts.append(_scaled_into_room(T(sh["floor_v"]), torch.max(ext[0] / span[0], ext[2] / span[2]), (lo + hi) / 2.0,
                                   torch.stack((ext[0] / 2.0, ext.new_zeros(()), ext[2] / 2.0))))
    cv = T(sh["ceil_v"])
    hi, lo = cv.max(0).values, cv.min(0).values
    span = hi - lo
    scale = torch.max(ext[0] / span[0], ext[2] / span[2])
    parts.append(_scaled_into_room(cv, scale, (lo + hi) / 2.0, torch.stack((ext[0] / 2.0, 0.5 * (scale * span)[1] + ext[1], ext[2] / 2.0))))
    return torch.cat(parts).contiguous()


def _model_index(models, i):
    """row i's entry of a per-row model choice (None, a short list or an entry < 0: model 0)"""
    if models is None or i >= len(models):
        return 0
    return max(int(models[i]), 0)


def assemble_scene(boxes, angles, class_names, bank, room_box, obj_size_target=None, models=None, shell=None):
    """diff_render.py:76-165 for one room: returns vertices_buf [1,V,3] (differentiable w.r.t. boxes / angles),
    face_buf [1,F,3] int32, class_ranges, obj sizes, size_loss.  ``boxes`` [n,6] in room-normalised units with the
    room row last, ``angles`` [n] in bins, ``room_box`` the frozen room row (6,).  ``models``: per row, the index of the class's
    model to place (``retrieve.retrieve_models``; None: model 0); ``shell``: the (wall, floor) entries (``place_shell``)."""
    dev = boxes.device
    ranges = {c: [] for c in _classes_of(bank)}
    ranges.update(wall=[], floor=[], ceiling=[])
    verts, faces, sizes, voff, foff = [], [], [], 0, 0
    size_loss = boxes.new_zeros(())
    k = 0
    for i, name in enumerate(class_names[:-1]):
        if name in DO_NOT_VIS or name not in bank.models:
            continue
        m = bank.model_list(name)[_model_index(models, i)]
        bmin, bmax = boxes[i][:3] * room_box[3:], boxes[i][3:] * room_box[3:]
        center, size = (bmax + bmin) / 2, bmax - bmin
        if obj_size_target is not None:
            size_loss = size_loss + F.mse_loss(size, obj_size_target[k])
        sizes.append(size.detach())
        k += 1
        theta = -angles[i] * (2 * math.pi / 24)
        msize, mcenter = m["bbox_max"] - m["bbox_min"], (m["bbox_min"] + m["bbox_max"]) / 2.0
        scale = torch.min(size / msize)
        c, s = torch.cos(theta), torch.sin(theta)
        zero, one = torch.zeros_like(c), torch.ones_like(c)
        rot = torch.stack([torch.stack([c, zero, s]), torch.stack([zero, one, zero]), torch.stack([-s, zero, c])])
        trans = center - scale * torch.matmul(rot, mcenter)
        v = torch.matmul(m["v"], (rot * scale).t()) + trans
        verts.append(v); faces.append(m["f"] + voff)
        ranges.setdefault(name, []).append([foff, foff + m["f"].shape[0]])
        voff += v.shape[0]; foff += m["f"].shape[0]
    # room shell for the frozen room box (diff_render.py:166-342; see place_shell)
    shell_v = place_shell(bank, room_box[3:].detach().cpu().tolist(), shell).to(dev)
    at = 0
    for nm, nv, f in shell_topology(bank, shell):
        verts.append(shell_v[at:at + nv]); faces.append(torch.from_numpy(f.astype(np.int32)).to(dev) + voff)
        ranges[nm].append([foff, foff + f.shape[0]])
        voff += nv; foff += f.shape[0]; at += nv
    return torch.cat(verts)[None], torch.cat(faces)[None], ranges, sizes, size_loss


def retrieve_choice(bank, boxes, class_names, rows=None):
    """The retrieval of models/diff_render.py:62,171,241 for row-concatenated rooms: ``boxes`` [N, 6] (room-normalised, every room's room
    row last), ``class_names`` the N rows' class names, ``rows`` the rooms' lengths (None: one room) ->
    (models int32 [N] on the boxes' device, -1 where nothing is retrieved; shells: [(wall, floor)] per room, None for a bank without a
    shell list).  One kernel launch each on the device (``retrieve.retrieve_models`` / ``retrieve_shell``); host tensors take the torch
    restatement - the CPU route of ``finetune_vae`` with an injected ``render_fn``."""
    table = bank.table
    boxes = boxes.detach().float()
    dev = boxes.device
    rows = [int(boxes.shape[0])] if rows is None else [int(n) for n in rows]
    index = {n: k for k, n in reversed(list(enumerate(table.vocab)))}
    cls = torch.tensor([index.get(n, -1) for n in class_names], dtype=torch.int32)
    last = np.cumsum(rows) - 1
    room_row = torch.from_numpy(np.repeat(last, rows).astype(np.int32))
    last_row = torch.from_numpy(last.astype(np.int32))
    if cls.numel() != boxes.shape[0] or int(room_row.numel()) != boxes.shape[0]:
        raise ValueError("class_names and rows must name every row of boxes")
    if boxes.is_cuda:
        if table.device != dev:
            table.to(dev)
        models = RT.retrieve_models(boxes, cls.to(dev), room_row.to(dev), table)
    else:
        models = RT.retrieve_models_torch(boxes, cls, room_row, table)
    shells, ratios = None, bank.shell_ratios
    if ratios is not None:
        fn = RT.retrieve_shell if boxes.is_cuda else RT.retrieve_shell_torch
        shells = [tuple(x) for x in fn(boxes, last_row.to(dev), ratios[0].to(dev), ratios[1].to(dev)).cpu().tolist()]
    return models, shells


_MESH_SOURCE = {"object_idx_to_name": None, "bank": None}


def configure_meshes(object_idx_to_name, bank=None, device="cuda"):
    """Stands in for the module globals of models/misc.py (:17-31: vocabulary + SUNCG model tables) that
    ``mesh_render_func`` reads.  ``bank`` defaults to one procedural model per furniture class."""
    _MESH_SOURCE["object_idx_to_name"] = list(object_idx_to_name)
    _MESH_SOURCE["bank"] = bank or MeshBank([n for n in set(object_idx_to_name) if n not in DO_NOT_VIS and n != "__room__"], device)


def mesh_render_func(boxes, angles, objs, model_ids_old=None, obj_size_target=None):
    """Same call contract as the reference (models/diff_render.py:48-435):
    ``boxes``: list of b tensors [6] (room-normalised, room row last), ``angles``: list of b scalar tensors (bins),
    ``objs``: list of b class indices -> ``(final[1,70,256,256], model_ids_return, obj_size_return, size_loss)``.
    First call (``model_ids_old is None``) caches the room box ("box_info"), the retrieved model id per object and the
    object sizes; later calls reuse them, overload the room box (:55-57) and add the size / wall-drift penalties
    (:98-100,160-165).  The first call retrieves every object's model from its own boxes (``retrieve_choice``: models/misc.py:34-64 over
    the bank's table) and returns the ids in ``model_ids_return[i]``, the chosen wall in ``["wall"]`` (and the floor in ``["floor"]``
    for a bank with a shell list); later calls place the meshes ``model_ids_old`` names, whatever their boxes have become."""
    src = _MESH_SOURCE
    if src["bank"] is None:
        raise RuntimeError("call refine.configure_meshes(object_idx_to_name) first (stands in for models/misc.py globals)")
    names, bank = src["object_idx_to_name"], src["bank"]
    boxes = list(boxes)
    dev = boxes[0].device
    model_ids_return, obj_size_return = {}, []
    old_wall = boxes[-1].clone()
    if model_ids_old is not None:
        boxes[-1] = torch.from_numpy(np.asarray(model_ids_old["box_info"])).float().to(dev)
    else:
        model_ids_return["box_info"] = boxes[-1].detach().cpu().numpy()
    class_names = [names[int(o)] for o in objs]
    table = bank.table
    if model_ids_old is None:
        # (:62,171,241) the retrieval on this call's own boxes; a row without a model to retrieve keeps the placeholder id
        models, shells = retrieve_choice(bank, torch.stack([b.detach() for b in boxes]), class_names)
        models = models.cpu().tolist()
        shell = shells[0] if shells is not None else None
        for i, n in enumerate(class_names[:-1]):
            model_ids_return[i] = table.id_of(table.vocab.index(n), models[i]) if models[i] >= 0 else n + "#0"
    else:
        # (:85-86,172-173,242-243) the meshes stay those of the first call
        models = []
        for i, n in enumerate(class_names[:-1]):
            ids = table.ids[table.vocab.index(n)] if n in table.vocab else []
            models.append(ids.index(model_ids_old[i]) if model_ids_old[i] in ids else 0)
        shell = None
        if getattr(bank, "shells", None):
            shell = (int(model_ids_old["wall"].get("index", 0)), int(model_ids_old.get("floor", {}).get("index", 0)))
    target = None
    if obj_size_target is not None:
        target = [torch.from_numpy(np.asarray(t)).float().to(dev) for t in obj_size_target[:-1]]
    v, f, ranges, sizes, size_loss = assemble_scene(torch.stack(boxes), torch.stack([a.reshape(()) for a in angles]).float(),
                                                    class_names, bank, boxes[-1].detach(), target, models=models, shell=shell)
    if obj_size_target is not None:
        size_loss = size_loss + F.mse_loss(old_wall, torch.from_numpy(np.asarray(obj_size_target[-1])).float().to(dev))
    else:
        obj_size_return = [x.cpu().numpy() for x in sizes] + [boxes[-1].detach().cpu().numpy()]
    if model_ids_old is None or obj_size_target is None:
        if shell is None:
            model_ids_return["wall"] = {"wall_bbox_min": [0.0, 0.0, 0.0], "wall_bbox_max": [float(x) for x in boxes[-1][3:]]}
        else:
            sw, sf = bank.shells[shell[0]], bank.shells[shell[1]]
            model_ids_return["wall"] = {"index": shell[0], "wall_bbox_min": sw["wall_bbox64"][0].tolist(), "wall_bbox_max": sw["wall_bbox64"][1].tolist()}
            model_ids_return["floor"] = {"index": shell[1], "floor_bbox_min": sf["floor_bbox64"][0].tolist(),
                                         "floor_bbox_max": sf["floor_bbox64"][1].tolist()}
    final = DR.scene_render(v, f, ranges, boxes[-1].detach())
    return final, model_ids_return, obj_size_return, size_loss


def refinement_loss(iter_image, target, target_container, size_loss):
    """test_render_refine.py:332-356 (target_container = per-scale argmax labels of the target, -100 where empty)."""
    iter_image = iter_image.clone()
    null = torch.sum(iter_image[:, 41:], dim=1) < 0.5
    last = iter_image[:, -1]
    iter_image[:, -1] = torch.where(null, torch.ones_like(last), last)
    depth_loss = F.l1_loss(psp_pool(iter_image[:, 41:]), psp_pool(target[:, 41:])) * 0.5
    sem = iter_image.new_zeros(())
    for pooled, tgt in zip(psp_pool(iter_image[:, 1:41], as_list=True), target_container):
        sem = sem + F.cross_entropy(pooled, tgt[:, 0]) / 800.0
    return depth_loss * 100 + sem * 100 + size_loss * 2.0, depth_loss, sem


def target_labels(target, sizes=(32, 48, 64, 96)):
    out = []
    for pooled in psp_pool(target[:, 1:41], sizes, as_list=True):
        flat = torch.argmax(pooled, dim=1, keepdim=True)
        flat[torch.sum(pooled, dim=1, keepdim=True) < 0.5] = -100
        out.append(flat.detach())
    return out


def _bilinear_taps(in_size, out_size, align_corners):
    """Source indices and weight of the upper neighbour exactly as upsample_bilinear2d derives them (fp32 arithmetic)."""
    dst = np.arange(out_size, dtype=np.float32)
    if align_corners:
        scale = np.float32(in_size - 1) / np.float32(out_size - 1) if out_size > 1 else np.float32(0)
        src = scale * dst
    else:
        src = np.maximum(np.float32(in_size) / np.float32(out_size) * (dst + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1.astype(np.int32), (src - i0.astype(np.float32)).astype(np.float32)


def pool_tap_sets(S, sizes=(32, 48, 64, 96)):
    """int64 [n_scales, P, 4]: the image indices the two resampling stages address for a pooled index - pool_kernel's
    ``{s1_i0[k], s1_i1[k] : k in {s2_k0[o], s2_k1[o]}}`` - whatever their weights (an exactly-hit sample still addresses its upper
    neighbour, with weight 0).  Rows and columns share the table; a pooled pixel's 16 taps are ``sets[s, oy] x sets[s, ox]``."""
    P = sizes[-1]
    out = np.zeros((len(sizes), P, 4), np.int64)
    for k, sz in enumerate(sizes):
        i0, i1, _ = _bilinear_taps(S, sz, True)
        k0, k1, _ = _bilinear_taps(sz, P, False)
        out[k] = np.stack([i0[k0], i1[k0], i0[k1], i1[k1]], 1)
    return torch.from_numpy(out)


def valid_pooled_torch(valid, sizes=(32, 48, 64, 96)):
    """``valid`` [B, S, S] (non-zero: the target means something here) -> bool [B, n_scales, P, P]: a pooled pixel is valid iff every
    image pixel of its tap set is (``pool_tap_sets``).  Integer-exact and separable: rows first, then columns."""
    v = valid != 0
    sets = pool_tap_sets(v.shape[-1], sizes).to(v.device)
    out = []
    for k in range(len(sizes)):
        rows = v[:, sets[k]].all(dim=2)                            # [B, P, S]: every addressed row valid, per image column
        out.append(rows[:, :, sets[k]].all(dim=3))                # [B, P, P]
    return torch.stack(out, 1)


def mask_counts_torch(valid, labels, per_room, sizes=(32, 48, 64, 96)):
    """What sln_refine_loss_mask derives, in torch ops: ``labels`` [B, n_scales, P, P] (as ``RefineLoss`` derives them, -100 = none) ->
    dict(valid_pooled uint8, labels int32, inv_count float32, depth_count int32 [2, B], mask_status int32 [B])."""
    vp = valid_pooled_torch(valid, sizes)
    lab = torch.where(vp, labels.to(torch.int32), torch.full_like(labels, -100, dtype=torch.int32))
    kept, ok = (lab >= 0).sum(dim=(2, 3)), vp.sum(dim=(2, 3))                                 # [B, n_scales]
    B = vp.shape[0]
    if not per_room:
        kept, ok = kept.sum(0, keepdim=True).expand(B, -1), ok.sum(0, keepdim=True).expand(B, -1)
    n = ok.sum(1)
    inv = 1.0 / (kept if per_room else kept[0]).to(torch.float32)
    status = (n == 0).to(torch.int32) | ((kept == 0).any(dim=1).to(torch.int32) << 1)
    return dict(valid_pooled=vp.to(torch.uint8), labels=lab, inv_count=inv,
                depth_count=torch.stack([n, (valid != 0).sum(dim=(1, 2))]).to(torch.int32), mask_status=status)


def refinement_loss_masked(iter_image, target, target_container, size_loss, valid, sizes=(32, 48, 64, 96)):
    """``refinement_loss`` under a validity mask (DESIGN §4 "Refinement loss under a validity mask"), in torch ops for any dtype and
    device - the CPU route and the yardstick of csrc/refine_loss.hip's masked kernels.  ``valid`` [B, S, S] (non-zero: the target means
    something at this pixel); ``target_container``: the per-scale labels as ``target_labels`` gives them.
      depth = 0.5 * sum over the VALID pooled pixels of |pool(iter) - pool(target)| / (29 * N), N the valid pooled pixels of all scales
              (0 when there is none); sem = sum_s CE_s / 800 over the labels of valid pooled pixels (a scale without one adds 0).
    Selects, never multiplies by 0: whatever ``target`` holds where ``valid`` is 0 (NaN and infinities included) reaches neither the
    value nor the gradient - an invalid image pixel is replaced by 0 before the target is pooled, which no valid pooled pixel reads.
    The iterate's planes enter detached at invalid pixels, so that their gradient is exactly 0 there whatever the dtype's rounding
    makes of a tap that lands on a sample (the definition's tap sets are float32's)."""
    v = (valid != 0)[:, None]
    vp = valid_pooled_torch(valid, sizes)                                                      # [B, ns, P, P]
    iter_image = torch.where(v, iter_image, iter_image.detach())
    null = torch.sum(iter_image[:, 41:], dim=1) < 0.5
    last = iter_image[:, -1]
    iter_image = torch.cat([iter_image[:, :-1], torch.where(null, torch.ones_like(last), last)[:, None]], 1)
    clean = torch.where(v, target, torch.zeros_like(target))
    B, ns, P = vp.shape[0], len(sizes), sizes[-1]
    diff = (psp_pool(iter_image[:, 41:], sizes) - psp_pool(clean[:, 41:], sizes)).abs().reshape(B, ns, -1, P, P)
    n = int(vp.sum())
    zero = (iter_image[:1, :1, :1, :1] * 0).sum()                    # (of the iterate: a loss without a term still has a - zero - gradient)
    depth_loss = torch.where(vp[:, :, None], diff, torch.zeros_like(diff)).sum() / (diff.shape[2] * n) * 0.5 if n > 0 else zero
    sem = zero
    for k, (pooled, tgt) in enumerate(zip(psp_pool(iter_image[:, 1:41], sizes, as_list=True), target_container)):
        lab = torch.where(vp[:, k], tgt[:, 0], torch.full_like(tgt[:, 0], -100))
        kept = int((lab >= 0).sum())
        if kept > 0:
            sem = sem + F.cross_entropy(pooled, lab, reduction="sum") / kept / 800.0
    return depth_loss * 100 + sem * 100 + size_loss * 2.0, depth_loss, sem


def check_mask(mask, shape, device, observed):
    """the ``mask=`` argument of the refinement entry points, refused before anything is launched: None, "readings" (needs ``observed``)
    or a uint8 / bool tensor of ``shape`` on ``device``"""
    if mask is None:
        return
    if isinstance(mask, str):
        if mask != "readings":
            raise ValueError("mask is None, 'readings' or a uint8 / bool tensor %s" % (list(shape),))
        if observed is None:
            raise ValueError("mask='readings' marks the pixels where the observed depth has a reading: it needs observed=")
        return
    if not torch.is_tensor(mask) or mask.dtype not in (torch.uint8, torch.bool):
        raise ValueError("mask: a uint8 or bool tensor expected (None and 'readings' are the other choices)")
    if tuple(mask.shape) != tuple(shape):
        raise ValueError("mask: shape %s is not %s" % (tuple(mask.shape), list(shape)))
    if mask.device != torch.device(device):
        raise ValueError("mask: a tensor on %s expected, got one on %s" % (device, mask.device))


def conf_pooled_torch(conf, sizes=(32, 48, 64, 96)):
    """``conf`` [B, S, S] uint8 -> uint8 [B, n_scales, P, P]: the minimum of the confidence over a pooled pixel's tap set
    (``pool_tap_sets``): a pooled pixel is as trustworthy as its least trusted tap.  Integer-exact and separable: rows first, then
    columns; for a {0, 255} image 255 * ``valid_pooled_torch``."""
    sets = pool_tap_sets(conf.shape[-1], sizes).to(conf.device)
    out = []
    for k in range(len(sizes)):
        rows = conf[:, sets[k]].amin(dim=2)                        # [B, P, S]
        out.append(rows[:, :, sets[k]].amin(dim=3))               # [B, P, P]
    return torch.stack(out, 1)


def confidence_counts_torch(conf, labels, per_room, sizes=(32, 48, 64, 96)):
    """What sln_refine_loss_confidence derives, in torch ops: ``labels`` [B, n_scales, P, P] (as ``RefineLoss`` derives them, -100 = none) ->
    dict(conf_pooled uint8, labels int32, inv_count float32, depth_count int32 [2, B], conf_sum int64 [2, B], mask_status int32 [B])."""
    cp = conf_pooled_torch(conf, sizes)
    c64 = cp.to(torch.int64)
    lab = torch.where(cp != 0, labels.to(torch.int32), torch.full_like(labels, -100, dtype=torch.int32))
    kept = torch.where(lab >= 0, c64, torch.zeros_like(c64)).sum(dim=(2, 3))                  # [B, n_scales]: sum of c over the kept labels
    ok, tot = (cp != 0).sum(dim=(2, 3)), c64.sum(dim=(2, 3))
    B = cp.shape[0]
    if not per_room:
        kept, ok, tot = (t.sum(0, keepdim=True).expand(B, -1) for t in (kept, ok, tot))
    n, sc = ok.sum(1), tot.sum(1)
    inv = 1.0 / ((kept if per_room else kept[0]).to(torch.float64) / 255.0).to(torch.float32)
    status = (sc == 0).to(torch.int32) | ((kept == 0).any(dim=1).to(torch.int32) << 1)
    return dict(conf_pooled=cp, labels=lab, inv_count=inv,
                depth_count=torch.stack([n, (conf != 0).sum(dim=(1, 2))]).to(torch.int32),
                conf_sum=torch.stack([sc, conf.to(torch.int64).sum(dim=(1, 2))]), mask_status=status)


def refinement_loss_confidence(iter_image, target, target_container, size_loss, conf, sizes=(32, 48, 64, 96)):
    """``refinement_loss`` under a per-pixel confidence of the target (DESIGN §4 "Refinement loss under per-pixel confidence"), in torch
    ops for any dtype and device - the CPU route and the yardstick of csrc/refine_loss.hip's confidence kernels.  ``conf`` [B, S, S]
    uint8 (0: the target says nothing here, 255: full trust); c the pooled confidence (``conf_pooled_torch``), w = c / 255:
      depth = 0.5 * sum over the pooled pixels with c > 0 of w |pool(iter) - pool(target)| / (29 * W), W = (sum of c) / 255 over all scales
              (0 when W is 0); sem = sum_s (sum of w * nll over the labels with c > 0) / W_s / 800 (a scale without one adds 0).
    Written as ``refinement_loss_masked``: selects, never multiplies by 0, and the iterate enters detached where ``conf`` is 0."""
    v = (conf != 0)[:, None]
    cp = conf_pooled_torch(conf, sizes)                                                        # [B, ns, P, P]
    vp = cp != 0
    iter_image = torch.where(v, iter_image, iter_image.detach())
    null = torch.sum(iter_image[:, 41:], dim=1) < 0.5
    last = iter_image[:, -1]
    iter_image = torch.cat([iter_image[:, :-1], torch.where(null, torch.ones_like(last), last)[:, None]], 1)
    clean = torch.where(v, target, torch.zeros_like(target))
    B, ns, P = vp.shape[0], len(sizes), sizes[-1]
    w = cp.to(iter_image.dtype) / 255
    diff = (psp_pool(iter_image[:, 41:], sizes) - psp_pool(clean[:, 41:], sizes)).abs().reshape(B, ns, -1, P, P)
    sc = int(cp.to(torch.int64).sum())
    zero = (iter_image[:1, :1, :1, :1] * 0).sum()                    # (of the iterate: a loss without a term still has a - zero - gradient)
    depth_loss = torch.where(vp[:, :, None], diff * w[:, :, None], torch.zeros_like(diff)).sum() / (diff.shape[2] * (sc / 255.0)) * 0.5 \
        if sc > 0 else zero
    sem = zero
    for k, (pooled, tgt) in enumerate(zip(psp_pool(iter_image[:, 1:41], sizes, as_list=True), target_container)):
        lab = torch.where(vp[:, k], tgt[:, 0], torch.full_like(tgt[:, 0], -100))
        kept = int(torch.where(lab >= 0, cp[:, k].to(torch.int64), torch.zeros_like(lab, dtype=torch.int64)).sum())
        if kept > 0:
            nll = F.cross_entropy(pooled, lab, reduction="none")                               # 0 at the ignored labels
            sem = sem + torch.where(lab >= 0, nll * w[:, k], torch.zeros_like(nll)).sum() / (kept / 255.0) / 800.0
    return depth_loss * 100 + sem * 100 + size_loss * 2.0, depth_loss, sem


def check_confidence(confidence, shape, device, mask=None, views=None):
    """the ``confidence=`` argument of the refinement entry points, refused before anything is launched: None, or a uint8 tensor of ``shape``
    on ``device`` (with ``views`` the shape carries the V axis).  ``confidence`` is the graded form of ``mask``: the two do not combine."""
    if confidence is None:
        return
    if mask is not None:
        raise ValueError("confidence is the graded form of mask (0: no say, 255: full trust): give one of the two")
    if not torch.is_tensor(confidence) or confidence.dtype != torch.uint8:
        raise ValueError("confidence: a uint8 tensor expected (0: the target says nothing here, 255: full trust)")
    if tuple(confidence.shape) != tuple(shape):
        if views is not None:
            raise ValueError("confidence: with views one image per view is expected, shape %s, got %s" % (list(shape), tuple(confidence.shape)))
        raise ValueError("confidence: shape %s is not %s" % (tuple(confidence.shape), list(shape)))
    if confidence.device != torch.device(device):
        raise ValueError("confidence: a tensor on %s expected, got one on %s" % (device, confidence.device))


def check_observed(observed, shape, device, cuda=True, choice=False):
    """the ``observed=`` argument of the refinement entry points, refused before anything is launched: None, or the pair (depth, uint8 labels),
    both tensors of ``shape`` = (rooms, S, S) on ``device``.  ``cuda``: the pair feeds ``ObservedTarget``, whose own check it passes (float32
    depth, a GPU); otherwise ``observed_target_torch``: any depth dtype, any device.  ``choice``: the caller asks for retrieved meshes."""
    if observed is None:
        return
    if choice:
        raise ValueError("observed targets show no meshes to retrieve: observed combines neither with retrieve=True nor with a bank that leaves a choice")
    if not isinstance(observed, (tuple, list)) or len(observed) != 2 or not all(torch.is_tensor(t) for t in observed):
        raise ValueError("observed is (depth %s float32, labels likewise uint8)" % (list(shape),))
    if cuda:
        OB.ObservedTarget.check_tensors(observed[0], observed[1], tuple(shape), device)
    elif any(tuple(t.shape) != tuple(shape) or t.device != torch.device(device) for t in observed) or observed[1].dtype != torch.uint8:
        raise ValueError("observed: depth and uint8 labels of shape %s on %s expected" % (list(shape), device))


def check_overlap(overlap_weight, overlap_rows, rooms):
    """the ``overlap_weight=`` / ``overlap_rows=`` arguments of the refinement entry points, refused before anything is launched.  ``rooms``:
    [(rows, class_names)] per room; ``overlap_rows``: None, or per room None or a bool sequence over the room's rows.  -> None with the weight at
    0 (nothing of the penalty exists), else per room the list of rows that collide: ``overlap_rows``' where given, otherwise the rows whose class
    is neither in DO_NOT_VIS nor the room's (``evaluate.collide_rows``); the room row - the last one - never collides."""
    w = float(overlap_weight)
    if not w >= 0.0:
        raise ValueError("overlap_weight must be >= 0, got %r" % (overlap_weight,))
    if overlap_rows is not None and len(overlap_rows) != len(rooms):
        raise ValueError("overlap_rows: one entry per room expected (None: the default rows of that room)")
    out = []
    for r, (n, names) in enumerate(rooms):
        rows = overlap_rows[r] if overlap_rows is not None else None
        if rows is not None:
            rows = [bool(v) for v in (rows.tolist() if torch.is_tensor(rows) else rows)]
            if len(rows) != n:
                raise ValueError("overlap_rows: room %d has %d rows, got %d flags" % (r, n, len(rows)))
        elif w > 0.0 and len(names) != n:
            raise ValueError("overlap_weight > 0 needs class_names that name every row of a room, or overlap_rows")
        elif w > 0.0:
            rows = [nm not in DO_NOT_VIS and nm != "__room__" for nm in names]
        if w > 0.0 and n > EV.MAX_ROOM_ROWS:
            raise ValueError("overlap_weight > 0: a room of more than %d rows" % EV.MAX_ROOM_ROWS)
        if rows:
            rows[-1] = False
        out.append(rows)
    return out if w > 0.0 else None


MAX_VIEWS = 64           # SLN_PLACE_MAX_VIEWS of include/sln_hip.h


def check_views(views, rooms=None, observed=None, mask=None, report=None, pictures=None, retrieve=False):
    """the ``views=`` argument of the refinement entry points, refused before anything is launched.  ``views``: None, or the cameras
    ``(K [R, V, 3, 3], Rm [R, V, 3, 3], t [R, V, 3])`` of V target views per room in ``get_cam_mat``'s convention, host or device tensors (or
    anything ``torch.as_tensor`` takes); ``rooms``: R, or None for the one-room form ``(K [V, 3, 3], Rm [V, 3, 3], t [V, 3])``.  -> None, or the
    three as contiguous float32 host tensors with the room axis.  Refused: anything else in shape, V > 64, a non-finite entry, tensors in
    ``observed`` or ``mask`` without the V axis (``[R, V, S, S]``; ``[V, S, S]`` in the one-room form), and ``report``, ``pictures`` or
    ``retrieve=True``, which do not combine with views."""
    if views is None:
        return None
    if not isinstance(views, (tuple, list)) or len(views) != 3:
        raise ValueError("views is (K [R, V, 3, 3], Rm [R, V, 3, 3], t [R, V, 3])")
    try:
        K, Rm, t = (torch.as_tensor(x).detach().to("cpu", torch.float32).contiguous() for x in views)
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError("views: three arrays of numbers expected (%s)" % e)
    lead = () if rooms is None else (int(rooms),)
    V = int(K.shape[len(lead)]) if K.dim() == len(lead) + 3 else -1
    want = [lead + (V, 3, 3), lead + (V, 3, 3), lead + (V, 3)]
    if V < 1 or [tuple(x.shape) for x in (K, Rm, t)] != want:
        raise ValueError("views: shapes %s are not K %s, Rm likewise, t %s with V >= 1 views" %
                         ([tuple(x.shape) for x in (K, Rm, t)], list(lead) + ["V", 3, 3], list(lead) + ["V", 3]))
    if V > MAX_VIEWS:
        raise ValueError("views: %d views per room, at most %d" % (V, MAX_VIEWS))
    if not all(bool(torch.isfinite(x).all()) for x in (K, Rm, t)):
        raise ValueError("views: a camera with a non-finite entry")
    for name, on in (("report", report is not None), ("pictures", pictures is not None), ("retrieve=True", bool(retrieve))):
        if on:
            raise ValueError("views does not combine with %s" % name)
    tensors = [("observed", x) for x in (observed if isinstance(observed, (tuple, list)) else ())] + [("mask", mask)]
    for name, x in tensors:
        if torch.is_tensor(x) and (x.dim() != len(lead) + 3 or tuple(x.shape[:len(lead) + 1]) != lead + (V,)):
            raise ValueError("%s: with views the V axis is needed, %s expected, got %s" % (name, list(lead) + [V, "S", "S"], tuple(x.shape)))
    if rooms is None:
        K, Rm, t = K[None], Rm[None], t[None]
    return K.contiguous(), Rm.contiguous(), t.contiguous()


POSE_KEYS = ("rot_step", "trans_step", "free", "start")
POSE_ORTHO_TOL = 1e-4    # a start rotation further than this from orthonormal (max |R R^T - I|) is refused


def check_poses(poses, views, rooms=None):
    """the ``poses=`` argument of the refinement entry points (DESIGN §4 "Camera poses of the target views"), refused before anything is
    launched.  ``poses``: None, or ``dict(rot_step=, trans_step=, free=None | bool [R, V], start=None | (Rm [R, V, 3, 3], t [R, V, 3]))``;
    ``views``: what ``check_views`` returned; ``rooms``: R, or None for the one-room form (``free`` [V], ``start`` ([V, 3, 3], [V, 3])).
    -> None, or dict(rot_step, trans_step: floats; free: bool [R, V] host tensor or None; start: (Rm, t) float32 host tensors - the camera
    table is float32 - or None).  Refused: poses without views, unknown keys, a negative or non-finite step, ``free`` that is no bool tensor
    [R, V], ``start`` that is no pair of float32 / float64 tensors of those shapes, a start rotation with max |R R^T - I| > 1e-4."""
    if poses is None:
        return None
    if views is None:
        raise ValueError("poses needs views: the poses refined are those of the target views")
    if not isinstance(poses, dict):
        raise ValueError("poses is a dict with the keys %s" % (POSE_KEYS,))
    unknown = sorted(set(poses) - set(POSE_KEYS))
    if unknown:
        raise ValueError("poses: unknown keys %s (known: %s)" % (unknown, POSE_KEYS))
    steps = {}
    for k in ("rot_step", "trans_step"):
        v = poses.get(k, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError("poses: %s is a finite number >= 0, got %r" % (k, v))
        steps[k] = float(v)
    R, V = int(views[0].shape[0]), int(views[0].shape[1])
    lead = (V,) if rooms is None else (R, V)
    free, start = poses.get("free"), poses.get("start")
    if free is not None:
        if not torch.is_tensor(free) or free.dtype != torch.bool or tuple(free.shape) != lead:
            raise ValueError("poses: free is a bool tensor %s" % (list(lead),))
        free = free.detach().cpu().reshape(R, V).contiguous()
    if start is not None:
        ok = isinstance(start, (tuple, list)) and len(start) == 2 and all(torch.is_tensor(x) and x.dtype in (torch.float32, torch.float64) for x in start)
        if not ok or tuple(start[0].shape) != lead + (3, 3) or tuple(start[1].shape) != lead + (3,):
            raise ValueError("poses: start is (Rm %s, t %s), float32 or float64 tensors" % (list(lead) + [3, 3], list(lead) + [3]))
        Rm, t = (x.detach().cpu().double().reshape((R, V) + tuple(x.shape[len(lead):])) for x in start)
        if not (bool(torch.isfinite(Rm).all()) and bool(torch.isfinite(t).all())):
            raise ValueError("poses: a start pose with a non-finite entry")
        off = float((torch.matmul(Rm, Rm.transpose(-1, -2)) - torch.eye(3, dtype=torch.float64)).abs().max())
        if off > POSE_ORTHO_TOL:
            raise ValueError("poses: a start rotation is not orthonormal (max |R R^T - I| = %.3g > %g)" % (off, POSE_ORTHO_TOL))
        start = (Rm.float().contiguous(), t.float().contiguous())
    return dict(rot_step=steps["rot_step"], trans_step=steps["trans_step"], free=free, start=start)


INTRINSICS_KEYS = ("focal_step", "center_step", "tie_focal", "free", "start")


def _check_pinhole(K, what):
    """a K the intrinsics' refinement can step: finite, zero skew (K[0, 1] = K[1, 0] = 0), fx, fy > 0, last row (0, 0, 1)"""
    if not bool(torch.isfinite(K).all()):
        raise ValueError("intrinsics: %s has a non-finite entry" % what)
    if bool((K[..., 0, 1] != 0).any()) or bool((K[..., 1, 0] != 0).any()):
        raise ValueError("intrinsics: %s has non-zero skew (K[0, 1], K[1, 0]): skew is not refined and the update assumes none" % what)
    if bool((K[..., 0, 0] <= 0).any()) or bool((K[..., 1, 1] <= 0).any()):
        raise ValueError("intrinsics: %s has a focal length that is not positive" % what)
    if not bool((K[..., 2, :] == torch.tensor([0.0, 0.0, 1.0], dtype=K.dtype)).all()):
        raise ValueError("intrinsics: the last row of %s is not (0, 0, 1)" % what)


def check_intrinsics(intrinsics, views, rooms=None):
    """the ``intrinsics=`` argument of the refinement entry points (DESIGN §4 "Intrinsics of the target views"), refused before anything is
    launched.  ``intrinsics``: None, or ``dict(focal_step=, center_step=, tie_focal=True, free=None | bool [R, V], start=None | K [R, V, 3, 3])``;
    ``views``: what ``check_views`` returned; ``rooms``: R, or None for the one-room form (``free`` [V], ``start`` [V, 3, 3]).
    -> None, or dict(focal_step, center_step: floats; tie_focal: bool; free: bool [R, V] host tensor or None; start: K float32 host tensor
    [R, V, 3, 3] - the camera table is float32 - or None).  Refused: intrinsics without views, unknown keys, a negative or non-finite step,
    a ``tie_focal`` that is no bool, ``free`` that is no bool tensor [R, V], ``start`` that is no float32 / float64 tensor [R, V, 3, 3], and a
    ``K`` - the views' or the start's - with a non-finite entry, non-zero skew, a focal length <= 0 or a last row other than (0, 0, 1)."""
    if intrinsics is None:
        return None
    if views is None:
        raise ValueError("intrinsics needs views: the intrinsics refined are those of the target views")
    if not isinstance(intrinsics, dict):
        raise ValueError("intrinsics is a dict with the keys %s" % (INTRINSICS_KEYS,))
    unknown = sorted(set(intrinsics) - set(INTRINSICS_KEYS))
    if unknown:
        raise ValueError("intrinsics: unknown keys %s (known: %s)" % (unknown, INTRINSICS_KEYS))
    steps = {}
    for k in ("focal_step", "center_step"):
        v = intrinsics.get(k, 0.0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError("intrinsics: %s is a finite number >= 0, got %r" % (k, v))
        steps[k] = float(v)
    tie = intrinsics.get("tie_focal", True)
    if not isinstance(tie, bool):
        raise ValueError("intrinsics: tie_focal is True or False, got %r" % (tie,))
    R, V = int(views[0].shape[0]), int(views[0].shape[1])
    lead = (V,) if rooms is None else (R, V)
    free, start = intrinsics.get("free"), intrinsics.get("start")
    if free is not None:
        if not torch.is_tensor(free) or free.dtype != torch.bool or tuple(free.shape) != lead:
            raise ValueError("intrinsics: free is a bool tensor %s" % (list(lead),))
        free = free.detach().cpu().reshape(R, V).contiguous()
    _check_pinhole(views[0], "a K of views")
    if start is not None:
        if not torch.is_tensor(start) or start.dtype not in (torch.float32, torch.float64) or tuple(start.shape) != lead + (3, 3):
            raise ValueError("intrinsics: start is K %s, a float32 or float64 tensor" % (list(lead) + [3, 3],))
        start = start.detach().cpu().reshape(R, V, 3, 3).float().contiguous()
        _check_pinhole(start, "a K of start")
    return dict(focal_step=steps["focal_step"], center_step=steps["center_step"], tie_focal=tie, free=free, start=start)


def _one_room_overlap(overlap_weight, overlap_rows, class_names, n, dev):
    """the one-room loops' checked penalty arguments -> None (weight 0), or the tensors of ``_overlap_term``: (collide uint8 [n], room_of_row
    int32 [n], room_id int32 [n]) on ``dev``"""
    rows = check_overlap(overlap_weight, None if overlap_rows is None else [overlap_rows], [(n, list(class_names))])
    if rows is None:
        return None
    return (torch.tensor(rows[0], dtype=torch.uint8, device=dev), torch.full((n,), n - 1, dtype=torch.int32, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev))


def _overlap_term(boxes_full, idx, tables, overlap_weight):
    """overlap_weight * penalty of one room's layout as a float32 scalar that autograd follows into ``boxes_full`` [n, 6] and ``idx`` [n]
    (``evaluate.overlap_penalty`` on checked tables: nothing is read back)"""
    collide, room_of_row, room_id = tables
    pen = EV._OverlapPenaltyFn.apply(boxes_full[None], idx[None], room_of_row, collide, room_id, 1)[0, 0]
    return (pen * float(overlap_weight)).float()


class _RefineLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, rl):
        image = image.contiguous()
        out = torch.empty((image.shape[0], 3) if rl.per_room else (3,), device=image.device)     # per_room: one (loss, depth, sem) triple per image
        _lib.check(_lib.lib().sln_refine_loss_forward(rl.desc, _lib.ptr(image), _lib.ptr(rl.target_depth), _lib.ptr(rl.labels),
                                                      _lib.ptr(rl.inv_count), _lib.ptr(rl.ws), _lib.ptr(out), _lib.current_stream_ptr()),
                   "sln_refine_loss_forward")
        ctx.rl, ctx.shape = rl, image.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        rl = ctx.rl
        g = torch.empty(ctx.shape, device=gout.device)
        # d/d(out[0]); out[1:] (the two parts) are reporting values.  per_room: ONE scale for every room (the rooms' losses are
        # independent objectives, each back-propagated with the same weight: element [0, 0])
        scale = gout.reshape(-1)[0:1].contiguous()
        _lib.check(_lib.lib().sln_refine_loss_backward(rl.desc, _lib.ptr(rl.ws), _lib.ptr(scale), _lib.ptr(g), _lib.current_stream_ptr()),
                   "sln_refine_loss_backward")
        return g, None


_REFINE_TABLES = {}          # (image size, scales, device) -> (device tables, longest CSR row): see RefineLoss.__init__


class RefineLoss:
    """``refinement_loss`` for a fixed target as two C calls (csrc/refine_loss.hip) instead of ~200 torch launches.
    ``rl(image)`` -> tensor [100*depth + 100*sem, depth, sem]; gradients flow to ``image`` through element 0.  The
    workspace holds d loss / d pooled between forward and backward: one outstanding forward per instance."""

    def __init__(self, target, sizes=(32, 48, 64, 96), per_room=False, valid=None, confidence=None):
        """``valid``: None, or [B, S, S] uint8 / bool on the target's device - the validity mask of the target (non-zero: the target
        means something at this pixel).  One ``sln_refine_loss_mask`` call derives ``valid_pooled`` [B, n_scales, P, P],
        masks ``labels``, recounts ``inv_count`` and fills ``mask_count`` [2, B] (valid pooled pixels the depth mean runs over, valid image
        pixels) and ``mask_status`` [B] (bit 0: no valid pooled pixel; bit 1: a scale without a label); all None without a mask.
        ``confidence``: None, or [B, S, S] uint8 on the target's device, not together with ``valid`` - the per-pixel confidence of the target
        (0: says nothing, 255: full trust).  One ``sln_refine_loss_confidence`` call derives ``conf_pooled`` [B, n_scales, P, P]
        (the minimum over a pooled pixel's taps), masks ``labels``, fills ``inv_count``, ``mask_count`` and ``mask_status`` as above (for the
        mask ``confidence != 0``) and ``conf_sum`` int64 [2, B] (pooled and image sums of the bytes); ``conf`` keeps the image."""
        self.per_room = bool(per_room)
        dev = target.device
        B, C, S, _ = target.shape
        check_mask(valid, (B, S, S), dev, None)
        check_confidence(confidence, (B, S, S), dev, valid)
        P, ns, pmax = sizes[-1], len(sizes), max(sizes)
        # the resampling tables depend on the geometry only (image size, scales), not on the room: built once per geometry and device
        # (python / numpy loops over 4 x 256 image rows: ~5 ms of the ~7 ms per-room set-up of the refinement loop)
        key = (S, tuple(sizes), str(dev))
        cached = _REFINE_TABLES.get(key)
        if cached is None:
            cached = _REFINE_TABLES[key] = self._build_tables(S, sizes, dev)
        self._keep, max_col = cached
        d = self._describe(B, S, P, C, ns, pmax, max_col)
        self._finish(d, target, B, S, P, C, ns, dev, valid, confidence)

    @staticmethod
    def _build_tables(S, sizes, dev):
        P, ns, pmax = sizes[-1], len(sizes), max(sizes)
        s2 = [np.zeros((ns, P), np.int32), np.zeros((ns, P), np.int32), np.zeros((ns, P), np.float32)]
        s1 = [np.zeros((ns, pmax), np.int32), np.zeros((ns, pmax), np.int32), np.zeros((ns, pmax), np.float32)]
        ptr, outs, ws_ = [], [], []
        for k, sz in enumerate(sizes):
            a = _bilinear_taps(S, sz, True)
            b = _bilinear_taps(sz, P, False)
            for dst, src in zip(s1, a):
                dst[k, :sz] = src
            for dst, src in zip(s2, b):
                dst[k] = src
            R1 = np.zeros((sz, S)); R2 = np.zeros((P, sz))
            np.add.at(R1, (np.arange(sz), a[0]), 1.0 - a[2].astype(np.float64)); np.add.at(R1, (np.arange(sz), a[1]), a[2].astype(np.float64))
            np.add.at(R2, (np.arange(P), b[0]), 1.0 - b[2].astype(np.float64)); np.add.at(R2, (np.arange(P), b[1]), b[2].astype(np.float64))
            comp = R2 @ R1                                             # [P, S]: pooled index <- image index
            base = sum(len(o) for o in outs)
            cp = [base]
            for y in range(S):
                nz = np.nonzero(comp[:, y])[0]
                outs.append(nz.astype(np.int32)); ws_.append(comp[nz, y].astype(np.float32))
                cp.append(cp[-1] + len(nz))
            ptr.append(np.asarray(cp, np.int32))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep = [t(x) for x in s2 + s1] + [t(np.stack(ptr)), t(np.concatenate(outs)), t(np.concatenate(ws_))]
        return keep, int(max(len(o) for o in outs))

    def _describe(self, B, S, P, C, ns, pmax, max_col):
        d = _lib.SlnRefineLoss()
        d.B, d.image_size, d.pooled_size, d.channels = B, S, P, C
        d.sem0, d.n_sem, d.dep0, d.n_dep, d.n_scales, d.stage1_stride = 1, 40, 41, C - 41, ns, pmax
        for name, buf in zip(("s2_k0", "s2_k1", "s2_l1", "s1_i0", "s1_i1", "s1_l1", "col_ptr", "col_out", "col_w"), self._keep):
            setattr(d, name, buf.data_ptr())
        d.max_col_entries = max_col
        d.per_room = int(getattr(self, "per_room", False))
        return d

    def _finish(self, d, target, B, S, P, C, ns, dev, valid=None, confidence=None):
        self.desc = d
        self.valid = self.valid_pooled = self.mask_count = self.mask_status = None
        self.conf = self.conf_pooled = self.conf_sum = None
        L = _lib.lib()
        self.ws = torch.empty(int(L.sln_refine_loss_workspace_bytes(B, S, P, ns, 40, C - 41)), dtype=torch.uint8, device=dev)
        _lib.check(L.sln_refine_loss_init(d, _lib.ptr(self.ws), _lib.current_stream_ptr()), "sln_refine_loss_init")
        # the target goes through the SAME resampling kernel as the iterates (no null-fill, test_render_refine.py:328-331):
        # where both images agree the pooled difference is exactly 0, as in the reference
        pooled = torch.empty(B, ns, C - 1, P, P, device=dev)
        _lib.check(L.sln_refine_pool(d, _lib.ptr(target.contiguous()), 0, _lib.ptr(self.ws), _lib.ptr(pooled), _lib.current_stream_ptr()),
                   "sln_refine_pool")
        self.target_depth = pooled[:, :, 40:].contiguous()                                              # [B, ns, 29, P, P]
        sem = pooled[:, :, :40]
        lab = torch.argmax(sem, dim=2)
        lab[sem.sum(dim=2) < 0.5] = -100                                                                # :341-343
        self.labels = lab.to(torch.int32).contiguous()                                                  # [B, ns, P, P]
        # per_room: every image is its own room - its cross-entropy means run over its own labels ([B, ns] counts)
        cnt = (lab >= 0).sum(dim=(2, 3) if self.per_room else (0, 2, 3)).to(torch.float32)
        self.inv_count = (1.0 / cnt).contiguous()                                                       # 1/0: nan loss, as torch's empty mean
        if valid is not None:
            # the mask (one call, four launches): pooled validity from pool_kernel's own tap indices, labels of invalid pooled pixels
            # to -100, the counts by integer sums on the device.  What the target holds under the mask stays where it is - in
            # target_depth and in the labels just derived - and is not read from here on.
            self.valid = (valid != 0).to(torch.uint8).contiguous()
            self.valid_pooled = torch.empty(B, ns, P, P, dtype=torch.uint8, device=dev)
            self.mask_count = torch.empty(2, B, dtype=torch.int32, device=dev)
            self.mask_status = torch.empty(B, dtype=torch.int32, device=dev)
            self.inv_count = torch.empty_like(self.inv_count)
            _lib.check(L.sln_refine_loss_mask(d, _lib.ptr(self.valid), _lib.ptr(self.labels), _lib.ptr(self.valid_pooled), _lib.ptr(self.inv_count),
                                              _lib.ptr(self.mask_count), _lib.ptr(self.mask_status), _lib.ptr(self.ws), _lib.current_stream_ptr()),
                       "sln_refine_loss_mask")
            d.valid_pooled, d.valid_image, d.depth_count = self.valid_pooled.data_ptr(), self.valid.data_ptr(), self.mask_count.data_ptr()
        if confidence is not None:
            # the confidence (one call, four launches): the mask's set-up with the minimum over the taps in place of the AND and integer
            # sums of the bytes beside the counts; the descriptor's mask fields then carry the graded forms
            self.conf = confidence.contiguous()
            self.conf_pooled = torch.empty(B, ns, P, P, dtype=torch.uint8, device=dev)
            self.mask_count = torch.empty(2, B, dtype=torch.int32, device=dev)
            self.conf_sum = torch.empty(2, B, dtype=torch.int64, device=dev)
            self.mask_status = torch.empty(B, dtype=torch.int32, device=dev)
            self.inv_count = torch.empty_like(self.inv_count)
            _lib.check(L.sln_refine_loss_confidence(d, _lib.ptr(self.conf), _lib.ptr(self.labels), _lib.ptr(self.conf_pooled), _lib.ptr(self.inv_count),
                                                    _lib.ptr(self.mask_count), _lib.ptr(self.conf_sum), _lib.ptr(self.mask_status), _lib.ptr(self.ws),
                                                    _lib.current_stream_ptr()), "sln_refine_loss_confidence")
            d.valid_pooled, d.valid_image, d.depth_count = self.conf_pooled.data_ptr(), self.conf.data_ptr(), self.mask_count.data_ptr()
            d.conf_sum = self.conf_sum.data_ptr()

    def pooled_ones(self):
        """[n_scales, P, P]: what the resampling kernel makes of an all-ones plane (one per geometry and device; see
        SlnRefineLoss::pooled_ones)"""
        d = self.desc
        key = ("ones", d.image_size, d.pooled_size, d.n_scales, d.stage1_stride, str(self.ws.device), self._keep[0].data_ptr())
        t = _REFINE_TABLES.get(key)
        if t is None:
            L, dev = _lib.lib(), self.ws.device
            d1 = type(d).from_buffer_copy(d)
            d1.B, d1.per_room, d1.live_planes, d1.pooled_ones = 1, 0, None, None
            d1.valid_pooled = d1.valid_image = d1.depth_count = d1.conf_sum = None
            C_, S, P, ns = d.channels, d.image_size, d.pooled_size, d.n_scales
            ws1 = torch.empty(int(L.sln_refine_loss_workspace_bytes(1, S, P, ns, 40, C_ - 41)), dtype=torch.uint8, device=dev)
            pooled = torch.empty(1, ns, C_ - 1, P, P, device=dev)
            _lib.check(L.sln_refine_pool(d1, _lib.ptr(torch.ones(1, C_, S, S, device=dev)), 0, _lib.ptr(ws1), _lib.ptr(pooled),
                                         _lib.current_stream_ptr()), "sln_refine_pool(ones)")
            t = _REFINE_TABLES[key] = pooled[0, :, 40].contiguous()
        return t

    def __call__(self, image):
        return _RefineLossFn.apply(image, self)


class _PlaceFn(torch.autograd.Function):
    """boxes [n,6], angles [n] -> (faces [2F,3,3] projected / culled / fill_back'ed, size_loss, sizes): csrc/placement.hip"""

    @staticmethod
    def forward(ctx, boxes, angles, scene, size_target):
        boxes, angles = boxes.contiguous().float(), angles.contiguous().float()
        dev = boxes.device
        fxyz = torch.empty(2 * scene.desc.F, 3, 3, device=dev)
        sizes = torch.empty(max(scene.n_vis, 1), 3, device=dev)
        sl = torch.empty(1, device=dev)
        tgt = size_target.contiguous().float() if size_target is not None else None
        _lib.check(_lib.lib().sln_place_forward(scene.desc, _lib.ptr(boxes), _lib.ptr(angles), _lib.ptr(tgt), _lib.ptr(fxyz), _lib.ptr(sizes),
                                                _lib.ptr(sl), _lib.current_stream_ptr()), "sln_place_forward")
        ctx.scene, ctx.tgt = scene, tgt
        ctx.save_for_backward(boxes, angles)
        sizes = sizes[:scene.n_vis]
        ctx.mark_non_differentiable(sizes)             # the reference detaches the cached sizes (diff_render.py:102)
        return fxyz, sl.reshape(()), sizes

    @staticmethod
    def backward(ctx, g_fxyz, g_sl, _g_sizes):
        boxes, angles = ctx.saved_tensors
        gb, ga = torch.empty_like(boxes), torch.empty_like(angles)
        _lib.check(_lib.lib().sln_place_backward(ctx.scene.desc, _lib.ptr(boxes), _lib.ptr(angles), _lib.ptr(ctx.tgt), _lib.ptr(g_fxyz.contiguous()),
                                                 _lib.ptr(g_sl.reshape(1).contiguous()), _lib.ptr(gb), _lib.ptr(ga), _lib.current_stream_ptr()),
                   "sln_place_backward")
        return gb, ga, None, None


class _HeadFn(torch.autograd.Function):
    """(boxes_pred [n,6], angles_pred [n,24], noise [n], box_last [6], angle_last [1]) -> (boxes_full [n,6], idx [n]): the
    soft-argmax, the noise, the two ``torch.cat`` with the frozen room row and - in backward - the ``fix_grad`` / ``quad_grad``
    hooks (testing/test_render_refine.py:20-25, 217-228, 296-306) as one launch each way (csrc/placement.hip) instead of ~25."""

    @staticmethod
    def forward(ctx, boxes_pred, angles_pred, noise, box_last, angle_last, beta):
        boxes_pred, angles_pred = boxes_pred.contiguous().float(), angles_pred.contiguous().float()
        n, na = angles_pred.shape
        boxes_full, idx = torch.empty_like(boxes_pred), torch.empty(n, device=boxes_pred.device)
        _lib.check(_lib.lib().sln_refine_head_forward(n, na, _lib.ptr(boxes_pred), _lib.ptr(angles_pred), _lib.ptr(noise), _lib.ptr(box_last),
                                                      _lib.ptr(angle_last), float(beta), _lib.ptr(boxes_full), _lib.ptr(idx),
                                                      _lib.current_stream_ptr()), "sln_refine_head_forward")
        ctx.save_for_backward(angles_pred)
        ctx.beta = float(beta)
        return boxes_full, idx

    @staticmethod
    def backward(ctx, g_boxes, g_idx):
        angles_pred, = ctx.saved_tensors
        n, na = angles_pred.shape
        gb, ga = torch.empty(n, 6, device=angles_pred.device), torch.empty_like(angles_pred)
        if g_boxes is None:
            g_boxes = torch.zeros(n, 6, device=angles_pred.device)
        if g_idx is None:
            g_idx = torch.zeros(n, device=angles_pred.device)
        _lib.check(_lib.lib().sln_refine_head_backward(n, na, _lib.ptr(angles_pred), _lib.ptr(g_boxes.contiguous()), _lib.ptr(g_idx.contiguous()),
                                                       ctx.beta, _lib.ptr(gb), _lib.ptr(ga), _lib.current_stream_ptr()),
                   "sln_refine_head_backward")
        return gb, ga, None, None, None, None


class RefineScene:
    """The same placement + render as ``assemble_scene`` + ``DR.scene_render`` with every per-object python loop of
    diff_render.py:76-159 turned into ONE batched tensor expression over the visible objects, and fixed tensor shapes:
    the near-plane cull (:346-356) degenerates the culled faces (all three corners collapse to a point, so they never
    cover a pixel) instead of compacting the face list.  Nothing in ``render`` synchronises with the host, which is what
    lets a whole refinement iteration be captured into one hipGraph (``finetune_vae_fast(..., capture=True)``).
    Built once per room: the room box is frozen (:55-60) and so are K, R, t."""

    def __init__(self, class_names, bank, room_box, image_size=DR.final_out, models=None, shell=None):
        """``models``: per row, the index of the class's model (``retrieve.retrieve_models``; None: model 0 everywhere);
        ``shell``: the (wall, floor) entries of the bank's shell list (``retrieve.retrieve_shell``; None: entry 0)"""
        dev = room_box.device
        self.image_size = image_size
        self.room = room_box.detach().clone()
        # everything that depends on the class list only (object meshes, face topology incl. the shell's, class tables) is built once
        # per (bank, class list) and shared by the rooms that use it - the refinement of a test set builds thousands of scenes from a
        # few dozen class lists; per room: the shell's vertices and the camera (round 5: 1.4 -> 0.3 ms per scene)
        cache = bank.__dict__.setdefault("_scene_cache", {})
        models = tuple(_model_index(models, i) for i in range(len(class_names) - 1))
        shell = None if shell is None else tuple(max(int(k), 0) for k in shell)
        self.models, self.shell = models, shell
        key = (tuple(class_names), str(dev), models, shell)
        st = cache.get(key)
        if st is None:
            st = cache[key] = self._static_part(class_names, bank, dev, models, shell)
        for k_, v_ in st.items():
            setattr(self, k_, v_)
        Vm = self._Vm
        room_host = [float(x) for x in room_box.detach().cpu().tolist()]           # one device -> host copy per scene
        room = room_host[3:]
        self.shell_v = place_shell(bank, room, shell).to(dev)                      # (the order of shell_topology / _static_part)
        Kc, Rc, tc = DR.get_cam_mat([room_host], "cpu")
        self.K, self.R, self.t = Kc.to(dev), Rc.to(dev), tc.to(dev)
        # descriptor of the fused placement kernels (csrc/placement.hip)
        self._keep = list(self._keep_static) + [self.shell_v]
        d = _lib.SlnPlacement()
        d.n, d.n_vis, d.Vm, d.Vs, d.F = len(class_names), self.n_vis, Vm, int(self.shell_v.shape[0]), int(self.faces.shape[0])
        for name, buf in zip(("vis", "model_v", "msize", "mcenter", "faces", "obj_face_ptr", "shell_v"), self._keep):
            setattr(d, name, buf.data_ptr())
        for name, vals in (("ext", room), ("K", Kc.reshape(-1).tolist()), ("R", Rc.reshape(-1).tolist()), ("t", tc.reshape(-1).tolist())):
            setattr(d, name, (type(getattr(d, name)))(*[float(x) for x in vals]))
        d.orig_size, d.proj_eps, d.cull_eps = float(DR.inter_out), 1e-9, float(DR.CULL_EPS)
        self.desc = d

    def with_view(self, K, R, t):
        """This scene seen through another camera (K [3, 3], R [3, 3], t [3] in ``get_cam_mat``'s convention, host or device): a shallow copy
        that shares every buffer, with ``K`` / ``R`` / ``t`` and the descriptor's camera replaced (``reproject.look_at_view``)."""
        dev = self.K.device
        Kc, Rc, tc = (torch.as_tensor(x, dtype=torch.float32).detach().cpu().reshape(s) for x, s in zip((K, R, t), ((1, 3, 3), (1, 3, 3), (1, 1, 3))))
        sc = copy.copy(self)
        sc.K, sc.R, sc.t = Kc.to(dev), Rc.to(dev), tc.to(dev)
        d = type(self.desc).from_buffer_copy(self.desc)
        for name, vals in (("K", Kc), ("R", Rc), ("t", tc)):
            setattr(d, name, (type(getattr(d, name)))(*[float(x) for x in vals.reshape(-1).tolist()]))
        sc.desc = d
        return sc

    @staticmethod
    def _static_part(class_names, bank, dev, choice=None, shell=None):
        vis = [i for i, nm in enumerate(class_names[:-1]) if nm not in DO_NOT_VIS and nm in bank.models]
        models = [bank.model_list(class_names[i])[_model_index(choice, i)] for i in vis]
        n_vis = len(vis)
        Vm = max([m["v"].shape[0] for m in models] + [1])
        mv = torch.zeros(max(n_vis, 1), Vm, 3, device=dev)
        for k, m in enumerate(models):
            mv[k, :m["v"].shape[0]] = m["v"]
        msize = torch.stack([m["bbox_max"] - m["bbox_min"] for m in models]) if models else torch.ones(1, 3, device=dev)
        mcenter = torch.stack([(m["bbox_min"] + m["bbox_max"]) / 2.0 for m in models]) if models else torch.zeros(1, 3, device=dev)
        ranges = {c: [] for c in _classes_of(bank)}
        ranges.update(wall=[], floor=[], ceiling=[])
        faces, foff = [], 0
        for k, (i, m) in enumerate(zip(vis, models)):
            faces.append(m["f"].long() + k * Vm)
            ranges.setdefault(class_names[i], []).append([foff, foff + m["f"].shape[0]]); foff += m["f"].shape[0]
        voff = n_vis * Vm
        for nm, nv, f in shell_topology(bank, shell):                          # topology only: the corners are the room's (place_shell)
            faces.append(torch.from_numpy(f.astype(np.int64)).to(dev) + voff)
            ranges[nm].append([foff, foff + f.shape[0]]); voff += nv; foff += f.shape[0]
        faces = torch.cat(faces)                                             # [F,3] into the flattened vertex list
        faces32 = faces.to(torch.int32)[None].contiguous()
        classes, chan, dch = DR.class_tables(ranges.keys())
        cls = torch.full((foff,), -1, dtype=torch.int32)
        for ci, name in enumerate(classes):
            for a, b in ranges[name]:
                cls[a:b] = ci
        vis_t = torch.tensor(vis, dtype=torch.int64, device=dev)
        counts = [m["f"].shape[0] for m in models]
        keep = [vis_t.to(torch.int32), mv.reshape(-1, 3).contiguous(), msize.contiguous(), mcenter.contiguous(), faces32[0].contiguous(),
                torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), device=dev)]
        return dict(vis=vis_t, n_vis=n_vis, _Vm=Vm, model_v=mv, msize=msize, mcenter=mcenter, faces=faces, faces32=faces32,
                    cls2=torch.cat((cls, cls))[None].contiguous().to(dev),          # fill_back doubles the faces
                    chan=torch.tensor(chan, dtype=torch.int32, device=dev), dch=torch.tensor(dch, dtype=torch.int32, device=dev),
                    _keep_static=keep)

    def place(self, boxes, angles):
        """-> vertices [1,V,3] (differentiable), object sizes [n_vis,3]"""
        ext = self.room[3:]
        b = boxes[self.vis]
        bmin, bmax = b[:, :3] * ext, b[:, 3:] * ext
        center, size = (bmax + bmin) / 2, bmax - bmin
        theta = -angles[self.vis] * (2 * math.pi / 24)
        scale = (size / self.msize).min(dim=1).values
        c, s_ = torch.cos(theta), torch.sin(theta)
        z, o = torch.zeros_like(c), torch.ones_like(c)
        rot = torch.stack([torch.stack([c, z, s_], 1), torch.stack([z, o, z], 1), torch.stack([-s_, z, c], 1)], 1)     # [n,3,3]
        trans = center - scale[:, None] * torch.matmul(rot, self.mcenter[:, :, None])[:, :, 0]
        v = torch.matmul(self.model_v, (rot * scale[:, None, None]).transpose(1, 2)) + trans[:, None, :]
        return torch.cat([v.reshape(-1, 3), self.shell_v])[None], size

    def render(self, boxes, angles, obj_size_target=None, fused=True):
        """-> final [1,70,is,is], size_loss, sizes.  ``fused``: placement, projection, cull and fill_back as ONE kernel each way
        (csrc/placement.hip) instead of the torch expression below (~100 launches per iteration with its autograd nodes)."""
        if fused:
            fxyz, size_loss, size = _PlaceFn.apply(boxes, angles, self, obj_size_target if self.n_vis else None)
            img = DR._SceneFn.apply(fxyz[None], self.cls2, self.chan, self.dch, self.image_size, 0.001)
            return img, size_loss, size
        verts, size = self.place(boxes, angles)
        size_loss = boxes.new_zeros(())
        if obj_size_target is not None and self.n_vis:
            size_loss = ((size - obj_size_target) ** 2).mean(1).sum()
        cam_z = (torch.matmul(verts, self.R.transpose(1, 2)) + self.t)[0, :, 2]
        culled = (cam_z[self.faces] < DR.CULL_EPS).any(1).detach()
        fxyz = DR.nr.project_faces(verts, self.faces32, self.K, self.R, self.t, DR.inter_out)[0]      # [F,3,3]
        fxyz = torch.where(culled[:, None, None], torch.zeros_like(fxyz), fxyz)
        fxyz = torch.cat((fxyz, torch.flip(fxyz, [1])), 0)[None]              # fill_back: corners (2, 1, 0)
        img = DR._SceneFn.apply(fxyz, self.cls2, self.chan, self.dch, self.image_size, 0.001)
        return img, size_loss, size


def room_start(model, room, noise_seed, iters, device, fp32=False):
    """A room's start as every loop draws it (test_render_refine.py:274-279, 304): the encoder (``model`` in eval mode), then on ONE CPU generator seeded
    with ``noise_seed`` (torch.manual_seed(13) in front of every trial) ``randn(mu.shape)`` for ``z0 = mu + randn * exp(0.5 logvar)`` and ``iters``
    times ``randn(n)`` - the soft-argmax noise of the iterations in the reference's order, up front so that a loop uploads it once.
    ``room``: dict with ``objs, triples, boxes, angles, attributes``; ``fp32``: the encoder's GEMMs in fp32 whatever ``model.gemm_precision``
    says.  -> (z0 [n, E] on ``device``, detached and the caller's own; noise rows [iters, n] on the host)"""
    with _precision(model, "fp32" if fp32 else None), torch.no_grad():
        mu, logvar = model.encoder(room["objs"], room["triples"], room["boxes"], room["angles"], room["attributes"])
    gen = torch.Generator(device="cpu").manual_seed(noise_seed)
    z0 = (mu + torch.randn(mu.shape, generator=gen).to(device) * torch.exp(0.5 * logvar)).detach()
    rows = [torch.randn(mu.shape[0], generator=gen) for _ in range(iters)]
    return z0, (torch.stack(rows) if rows else torch.zeros(0, mu.shape[0]))


def _shared_class_tables(scenes):
    """(chan, dch) of the scenes of one batch, which must share them"""
    chan, dch = scenes[0].chan, scenes[0].dch
    for sc in scenes[1:]:
        if not (torch.equal(sc.chan, chan) and torch.equal(sc.dch, dch)):
            raise _lib.SlnError("rooms of one batch must share the class tables")
    return chan, dch


def room_target(room, bank, image_size, models=None, shell=None, observed=False):
    """A room's target for the device loops: the scene of the ground-truth rows (``models`` / ``shell``: what ``retrieve_choice`` picked for them)
    and its render.  ``observed``: the caller builds the targets of its rooms with one ``ObservedTarget`` call - then only the placement
    runs, for the sizes.  -> (scene, target [1, C, S, S] or None, sizes [n_vis, 3] of the caller's own)"""
    scene = RefineScene(room["class_names"], bank, room["boxes"][-1].detach().clone(), image_size, models=models, shell=shell)
    with torch.no_grad():
        if observed:
            target, (_, _, sizes) = None, _PlaceFn.apply(room["boxes"], room["angles"].float(), scene, None)
        else:
            target, _, sizes = scene.render(room["boxes"], room["angles"].float())
    return scene, target, sizes.detach().clone().contiguous()


def valid_and_labels(mask, target, labels=True):
    """A checked ``mask`` and the built ``target`` [B, C, S, S] -> (valid uint8 [B, S, S] - 'readings': where plane 0, the cleaned depth, has a
    reading - or None without a mask; the per-scale labels of the target cleaned under it, None with ``labels`` off: ``RefineLoss`` derives its own)"""
    valid = None
    if mask is not None:
        valid = ((target[:, 0] >= 0) if isinstance(mask, str) else (mask != 0)).to(torch.uint8).contiguous()
    if not labels:
        return valid, None
    return valid, target_labels(target if valid is None else torch.where(valid[:, None] != 0, target, torch.zeros_like(target)))


def confidence_and_labels(confidence, target, labels=True):
    """``valid_and_labels`` for a checked ``confidence`` [B, S, S]: -> (the bytes, contiguous; the per-scale labels of the target cleaned under
    ``confidence > 0``, None with ``labels`` off)"""
    conf = confidence.contiguous()
    if not labels:
        return conf, None
    return conf, target_labels(torch.where(conf[:, None] != 0, target, torch.zeros_like(target)))


def parse_schedule(spec, iters, name):
    """The iterations a per-iteration extra (``report``, ``pictures``) runs in: ``spec`` None, "ends" (0 and the last), "all" or an
    iterable of iteration numbers in [0, max(iters, 1)) -> None, or (sorted tuple of iteration numbers, is it "all")."""
    if spec is None:
        return None
    n = max(int(iters), 1)
    named = {"all": range(n), "ends": (0, n - 1)}
    if isinstance(spec, str) and spec not in named:
        raise ValueError("%s is None, 'ends', 'all' or an iterable of iteration numbers" % name)
    at = tuple(sorted(set(named[spec] if isinstance(spec, str) else [int(k) for k in spec])))
    if any(k < 0 or k >= n for k in at):
        raise ValueError("%s names an iteration outside [0, %d)" % (name, iters))
    return at, isinstance(spec, str) and spec == "all"


class GraphStep:
    """One step of a loop as a hipGraph.  ``run(step)``: the first call runs ``step()`` on a side stream (the warm-up outside the capture:
    allocator, lazy kernel attributes), then records a second ``step()`` into the graph; every later call replays it.  -> what the
    step returned: the warm-up's the first time, the recorded call's (the graph's static outputs) from then on."""
    graph = out = None

    def run(self, step):
        if self.graph is not None:
            self.graph.replay()
            return self.out
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = step()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = step()
        return out


def cut_ranges(ranges, offsets=None, lengths=None):
    """``ranges`` [(offset, length)] of a flat float buffer minus the tensors at ``offsets`` of ``lengths`` -> what is left, in order.  A length
    is padded up to 64 floats when every offset is a multiple of 64 (the flat parameter layout pads every tensor to 64 floats, nothing lives
    in the pad), otherwise to 4.  A cut must start on a multiple of 4 (16 bytes) and not before the position reached inside its range."""
    if not offsets:
        return list(ranges)
    al = 64 if all(o % 64 == 0 for o in offsets) else 4
    cut = sorted((int(o), -(-int(n) // al) * al) for o, n in zip(offsets, lengths))
    out = []
    for a, n in ranges:
        pos, end = a, a + n
        for c0, cn in cut:
            if c0 + cn <= pos or c0 >= end:
                continue
            if c0 % 4 or c0 < pos:
                raise _lib.SlnError("a fused parameter tensor does not start on a 16-byte boundary of the decoder run")
            if c0 > pos:
                out.append((pos, c0 - pos))
            pos = c0 + cn
        if pos < end:
            out.append((pos, end - pos))
    return out


def _one_room_arguments(observed, mask, S, dev, cuda, bank=None):
    """``observed`` / ``mask`` of the one-room loops, brought from [S, S] to [1, S, S] and checked before anything is launched"""
    lift = lambda t: t[None] if torch.is_tensor(t) and t.dim() == 2 else t
    observed, mask = tuple(lift(t) for t in observed) if isinstance(observed, (tuple, list)) else observed, lift(mask)
    check_observed(observed, (1, S, S), dev, cuda, choice=bank is not None and bank.has_choice())
    check_mask(mask, (1, S, S), dev, observed)
    return observed, mask


def _one_room_confidence(confidence, mask, S, dev):
    """``confidence`` of the one-room loops, brought from [S, S] to [1, S, S] and checked before anything is launched"""
    if torch.is_tensor(confidence) and confidence.dim() == 2:
        confidence = confidence[None]
    check_confidence(confidence, (1, S, S), dev, mask)
    return confidence


def finetune_vae_fast(model, objs, triples, boxes_gt, angles_gt, attributes, class_names, iters=60, bank=None, learning_rate=1e-4,
                      noise_seed=13, image_size=256, capture=False, log=None, fused_loss=True, fused_head=True, observed=None, mask=None,
                      overlap_weight=0.0, overlap_rows=None, confidence=None):
    """``finetune_vae`` with the batched ``RefineScene`` and no per-iteration python optimiser objects: the reference builds a
    NEW SGD(momentum=0.1, nesterov) every iteration (test_render_refine.py:286-292), so its step is exactly
    ``p -= lr * (1 + momentum) * grad``; that closed form is applied to ``z`` (lr 2e-4) and to the flat parameter buffer
    (lr ``learning_rate``/10).  ``fused_loss``: the PSP-pool / L1 / cross-entropy block runs as ``RefineLoss`` (two C calls)
    instead of torch ops; ``fused_head``: the soft-argmax / noise / concatenation glue and the two gradient hooks as one launch
    each way (``_HeadFn``) and both parameter updates plus the gradient zero-fill as one launch (``sln_refine_sgd``).
    ``capture=True`` records one iteration (decoder, placement, fused render, PSP losses, backward, both updates) into a hipGraph and
    replays it (``GraphStep``).
    ``observed``: None, or ``(depth [S, S] or [1, S, S] float32, labels likewise uint8)`` on the device - the target is built from this
    observation with one ``ObservedTarget`` call on the room's class tables instead of rendered from ``boxes_gt`` (``RefineBatch``'s
    ``observed``, for one room).  ``mask``: None, "readings" or a uint8 / bool tensor [S, S] or [1, S, S] - the loss under a validity mask
    (``RefineBatch``'s ``mask``).  ``confidence``: None, or a uint8 tensor [S, S] or [1, S, S], not together with ``mask`` - the loss under a
    per-pixel confidence of the target (``RefineBatch``'s ``confidence``).  ``overlap_weight`` / ``overlap_rows`` (a bool sequence over the rows):
    ``RefineBatch``'s, for one room - the loss gains ``overlap_weight * evaluate.overlap_penalty`` of the iterate, followed by autograd.
    Returns (losses [iters] tensor on the device, (boxes_pred, angle_idx)).  ``log``: called once per iteration, the captured one included."""
    dev, S = boxes_gt.device, int(image_size)
    observed, mask = _one_room_arguments(observed, mask, S, dev, True, bank)
    confidence = _one_room_confidence(confidence, mask, S, dev)
    overlap = _one_room_overlap(overlap_weight, overlap_rows, class_names, int(boxes_gt.shape[0]), dev)
    bank = bank or MeshBank([n for n in set(class_names) if n not in DO_NOT_VIS], dev)
    room = dict(objs=objs, triples=triples, boxes=boxes_gt, angles=angles_gt, attributes=attributes, class_names=class_names)
    model.eval()
    # the soft-argmax noise of every iteration is uploaded once: a per-iteration host-to-device copy would block the host and leave
    # the GPU idle between two iterations
    z, noise_all = room_start(model, room, noise_seed, iters, dev)
    z, noise_all = z.requires_grad_(True), noise_all.to(dev)
    # the target shows the meshes retrieved for the ground-truth boxes (test_render_refine.py:319), the iterates those retrieved for
    # iteration 0's boxes (:324-326) - two scenes when the bank leaves a choice
    models_gt, shell = None, None
    if bank.has_choice():
        models_gt, shells = retrieve_choice(bank, boxes_gt, class_names)
        models_gt, shell = models_gt.cpu().tolist(), (shells[0] if shells is not None else None)
    target_scene, target, size_target = room_target(room, bank, S, models_gt, shell, observed is not None)      # (size_target: a buffer, filled below)
    scene = target_scene
    if observed is not None:                                           # the target from the observation (csrc/observed_target.hip)
        target = OB.ObservedTarget(scene.chan, scene.dch, S, batch=1, device=dev, nch=DR.N_SCENE_CHANNELS)(*observed)[0]
    valid, labels = valid_and_labels(mask, target, labels=not fused_loss)
    conf = None
    if confidence is not None:
        conf, labels = confidence_and_labels(confidence, target, labels=not fused_loss)
    fused = RefineLoss(target, valid=valid, confidence=conf) if fused_loss else None    # the PSP / L1 / cross-entropy block as two C calls
    noise = torch.zeros(boxes_gt.shape[0], device=dev)
    losses = torch.zeros(iters, device=dev)
    flat, flat_grad, state = model.flat_params, model.flat_grads, {}
    box_last, angle_last = boxes_gt[-1].detach().float().contiguous(), angles_gt[-1:].detach().float().contiguous()
    if fused_head:
        flat_grad.zero_()                                  # from here on the update kernel leaves the gradient buffer zeroed
    if iters > 0 and scene.n_vis:
        # the size penalty holds the objects to the sizes of the FIRST iterate (see ``RefineBatch._first_iterate_sizes``): one decoder +
        # placement pass with iteration 0's z, parameters and noise row
        with torch.no_grad():
            bp0, ap0 = model.decoder(z, objs, triples, attributes)
            b0 = torch.cat([bp0[:-1], boxes_gt[-1:]], 0)
            i0 = torch.cat([(softargmax(ap0, sum_dim=1) + noise_all[0] / 10.0)[:-1], angles_gt[-1:].float()], 0)
            size_target.copy_(_PlaceFn.apply(b0, i0, target_scene, None)[2])              # (sizes do not depend on the model)
            if bank.has_choice():
                scene = RefineScene(class_names, bank, target_scene.room, S, models=retrieve_choice(bank, b0, class_names)[0].cpu().tolist(),
                                    shell=shell)

    def iteration():
        boxes_pred, angles_pred = model.decoder(z, objs, triples, attributes)
        if fused_head:
            boxes_full, idx = _HeadFn.apply(boxes_pred, angles_pred, noise, box_last, angle_last, 2.0)
        else:
            boxes_pred.register_hook(fix_grad)
            boxes_full = torch.cat([boxes_pred[:-1], boxes_gt[-1:]], 0)
            idx = softargmax(angles_pred, sum_dim=1) + noise / 10.0
            idx.register_hook(quad_grad)
            idx = torch.cat([idx[:-1], angles_gt[-1:].float()], 0)
        image, size_loss, _ = scene.render(boxes_full, idx, size_target)
        if fused is not None:
            loss = torch.add(fused(image)[0], size_loss, alpha=2.0)
        elif conf is not None:
            loss, _, _ = refinement_loss_confidence(image, target, labels, size_loss, conf)
        elif valid is not None:
            loss, _, _ = refinement_loss_masked(image, target, labels, size_loss, valid)
        else:
            loss, _, _ = refinement_loss(image, target, labels, size_loss)
        if overlap is not None:
            loss = loss + _overlap_term(boxes_full, idx, overlap, overlap_weight)
        z.grad = None
        if not fused_head:
            flat_grad.zero_()
        loss.backward()
        with torch.no_grad():
            if fused_head:
                _lib.check(_lib.lib().sln_refine_sgd(_lib.ptr(flat), _lib.ptr(flat_grad), flat.numel(), (learning_rate / 10.0) * 1.1,
                                                     _lib.ptr(z), _lib.ptr(z.grad), z.numel(), 2e-4 * 1.1, _lib.current_stream_ptr()),
                           "sln_refine_sgd")
            else:
                z.add_(z.grad, alpha=-2e-4 * 1.1)
                flat.add_(flat_grad, alpha=-(learning_rate / 10.0) * 1.1)
        model.params_changed()
        state["boxes"], state["idx"] = boxes_full.detach(), idx.detach()
        return loss.detach()

    graph = GraphStep()
    for k in range(iters):
        noise.copy_(noise_all[k])
        losses[k] = graph.run(iteration) if capture else iteration()
        if log:
            log("iter %d: loss %.4f" % (k, float(losses[k])))
    return losses, (state["boxes"], state["idx"])


PictureSet = collections.namedtuple("PictureSet", "depth8 labels rgb status iterations")


class RefineBatch:
    """R rooms in flight: one refinement iteration of R independent rooms (testing/test_render_refine.py:250-263 runs its trials
    one after the other; each reloads the checkpoint, ``model.eval()``, and :279-359 steps ``z`` AND its own copy of the parameters)
    as ONE sequence of launches - no autograd graph, no per-room python:

        decoder of all rooms (sln_vae_group_decoder: R parameter copies, one launch per step) -> soft-argmax / noise / frozen room
        row (sln_refine_head_forward_rooms) -> placement + projection + cull + fill_back (sln_place_forward_rooms) -> fused scene
        pass over the R padded face lists (sln_scene_forward) -> PSP / L1 / cross-entropy per room (SlnRefineLoss.per_room) ->
        the same chain backwards -> decoder backward of all rooms -> SGD on every room's parameter copy and on z (one launch).

    ``rooms``: list of dicts with ``objs, triples, boxes, angles, attributes`` (one room's collated graph, room row last) and
    ``class_names``.  Every room starts from ``model``'s parameters (the checkpoint), encoded with ``model`` in eval mode.
    A room's numbers do not depend on the other rooms of the batch: the kernels are the single-room ones over a (room) grid axis.
    After ``run(iters)``: ``losses`` [iters, R], ``boxes`` / ``idx`` (row-concatenated, ``row0`` / ``rows`` per room), ``params``
    [R, n_flat] the fine-tuned copies, ``z`` the refined latents.

    ``report``: None (default: nothing below exists, the launches are those above), "ends" (iterations 0 and the last: what the
    reference dumps, test_render_refine.py:369), "all", or an iterable of iteration numbers.  A reported iteration issues two more
    calls - sln_layout_cuboid_iou over all rooms' rows after the head (boxes / idx of the iterate against the ground truth, :360-368)
    and sln_refine_report after the loss forward - and fills ``report[k]`` [R, 3] = (mean IoU of the room's visible rows,
    depth_l1 at full resolution, cross-entropy of the last scale; :371-372); rows of unreported iterations stay NaN.  Nothing is
    read back and nothing allocated inside an iteration.

    ``pictures``: None (default: nothing below exists, the launches are those above), "ends" (:369), "all", or an iterable of iteration
    numbers - what the reference's ``save_images`` calls show (:320, :377; host/scene_pictures.py).  A pictured iteration issues
    sln_scene_pictures (three launches) on ``image`` with ``live`` after the loss forward and fills slot j of ``pictures.depth8`` /
    ``labels`` [n_pictured, R, S, S], ``rgb`` [n_pictured, R, S, S, 3] and ``status`` [n_pictured, R]; ``pictures.iterations[j]`` names the
    iteration.  ``target_pictures`` (``scene_pictures.Pictures``, [R, S, S(, 3)]) is filled once at set-up from the target renders.
    Needs image_size % 4 == 0.

    ``retrieve``: False (default: every row shows model 0 of its class, the launches are those above), or True - the targets show the
    models retrieved for the ground-truth boxes (one ``retrieve.retrieve_models`` launch over all rooms' rows at construction,
    :319), the iterates those retrieved for the FIRST iterate's boxes (one launch over ``boxes`` behind ``_first_iterate_sizes``' forward
    in the first ``run()``, :324-326; read back - set-up, outside any capture - after which the iterates' scenes are built and bound,
    ``_bind_scenes``), frozen from then on.  ``target_models`` / ``models`` (int32 [N], -1 where nothing is retrieved) and
    ``model_ids()`` expose the choice; a bank with a shell list gets its (wall, floor) entries per room the same way.

    ``observed``: None (default: every room's target is the render of its own ``boxes``, the launches are those above), or
    ``(depth [R, S, S] float32, labels [R, S, S] uint8)`` on the device - one observation per room of the refinement camera
    (``get_cam_mat`` of the room row; host/observe.py) from which ONE ``ObservedTarget`` call on the batch's class tables builds the R
    targets; nothing is rendered from ``rm["boxes"]``.  The encoder start, the frozen room row, the camera and the size targets stay
    ``rm[...]``'s; ``report``'s depth term and ``target_pictures`` read the observed targets; ``target_status`` [R] holds the status
    words of the observations (None without ``observed``).  Does not combine with ``retrieve=True``.

    ``mask``: None (default: the loss reads every pixel of the targets, the launches are those above), "readings" (needs ``observed``: a
    pixel is valid where the cleaned depth has a reading, ``d0 >= 0`` in plane 0 of the built target - the holes of a reprojected frame
    are not), or a uint8 / bool tensor [R, S, S] on the device (non-zero: valid; works with rendered targets too).  The loss then runs
    under the validity mask (``RefineLoss(valid=)``): the depth term and its gradient over the valid pooled pixels only, the
    labels of the others ignored, ``report``'s depth_l1 over the valid image pixels.  ``mask_status`` [R] int32 (None without a mask):
    bit 0 - the room has no valid pooled pixel (its depth term is 0), bit 1 - one of its scales keeps no label.

    ``confidence``: None (default: nothing below exists), or a uint8 tensor [R, S, S] on the device, not together with ``mask`` - the per-pixel
    confidence of the targets (0: the target says nothing here, as ``mask`` 0; 255: full trust; ``reproject.ObservedFuser.confidence`` builds
    one from the fusion's agreement counts).  The loss then runs under it (``RefineLoss(confidence=)``, DESIGN §4 "Refinement loss under
    per-pixel confidence"): a pooled pixel weighs c / 255 with c the minimum of the bytes over its taps, every mean is divided by the sum
    of its weights, ``report``'s depth_l1 likewise over the image.  No launch more per iteration than with ``mask``.  A {0, 255} tensor
    gives the bits of ``mask``; a constant one cancels (each image is normalised by its own sum): confidence says which pixels of an
    image matter, not which image.  ``mask_status`` as with ``mask``.  With ``views``: ``[R, V, S, S]``.

    ``overlap_weight``: 0.0 (default: nothing below exists, the launches are those above), or a weight > 0 - the loss of a room becomes
    ``... + 2 size_loss + overlap_weight * penalty`` with ``penalty`` the summed intersection volume of the room's colliding furniture
    (``evaluate.overlap_penalty``): what keeps an object whose hidden side the target does not show out of its neighbour.  The head
    then runs in launches of its own (the route of rooms above 128 rows) and one sln_layout_overlap_penalty call over all rooms' rows adds the
    penalty's gradient onto the placement's in front of the head's backward (the ``fix_grad`` / ``quad_grad`` hooks see it); ``overlap``
    [iters, R] float64 holds the unweighted penalty of every iteration (None with the weight at 0).  ``overlap_rows``: None, or per room None
    or a bool sequence over the room's rows that replaces the default choice of colliding rows (the class is not in DO_NOT_VIS; needs
    ``class_names`` that name every row) - to exempt a lamp that a graph places "inside" a shelf; a room row never collides.

    ``views``: None (default: every room is refined against its one refinement view, the launches are those above), or the cameras
    ``(K [R, V, 3, 3], Rm [R, V, 3, 3], t [R, V, 3])`` of V target views per room, host or device, in ``get_cam_mat``'s convention
    (``reproject.refine_view`` / ``look_at_view``; DESIGN §4 "Several target views per room").  The views REPLACE the room's camera: view 0
    need not be ``get_cam_mat``'s.  Image ``b = r * V + v``: the placement is done once per room and projected through its V cameras
    (sln_place_forward_views / sln_place_backward_views instead of the ``_rooms`` pair, the head in launches of its own), the scene pass and
    the loss run over R * V images, and a room's loss is ``mean_v L[r, v] + 2 size_loss`` (``+ overlap_weight * penalty``) - every image's
    gradient is scaled by float32(1 / V).  The targets are the renders of ``rm["boxes"]`` through each view's camera
    (``RefineScene.with_view``), or ``observed`` frames: ``observed`` and a tensor ``mask`` are then ``[R, V, S, S]``, ``target_status`` and
    ``mask_status`` ``[R, V]``.  A room with fewer than V views passes an all-zero ``mask`` for the missing ones - the divisor stays V;
    there is no other ragged form.  The camera table is uploaded once at set-up.  Out of scope, and refused: ``report``, ``pictures`` and
    ``retrieve=True`` together with ``views``.

    ``poses``: None (default: the views' cameras are exact, the launches are those above and the camera table stays the one uploaded at
    set-up), or ``dict(rot_step=, trans_step=, free=None | bool [R, V], start=None | (Rm [R, V, 3, 3], t [R, V, 3]))`` - needs ``views``
    (DESIGN §4 "Camera poses of the target views").  Every iteration then issues one more launch behind sln_place_backward_views,
    sln_place_pose_step_views: per (room, view) the gradient of the room's loss with respect to a rigid motion of the camera frame
    (``pose_grad`` [iters, R, V, 6] float64: d omega, d tau - recorded on the device), and for the views marked ``free`` (None: all) the step
    ``omega = -rot_step dL/domega``, ``tau = -trans_step dL/dtau`` on a float64 master copy of the poses, whose float32 rounding is the
    camera table the next iteration projects through.  ``K`` is not refined.  ``start``: the cameras the loop begins from when they
    differ from those the targets were rendered through (``views``) - the synthetic experiment; with ``observed`` there is nothing to
    distinguish, and ``views`` are the start.  After ``run()``: ``poses()`` -> (Rm, t) float64, ``pose_error(Rm_ref, t_ref)``.

    ``intrinsics``: None (default: ``K`` of every view is exact; the launches and the bits are those above), or ``dict(focal_step=,
    center_step=, tie_focal=True, free=None | bool [R, V], start=None | K [R, V, 3, 3])`` - needs ``views``, combines with ``poses`` or stands
    alone (DESIGN §4 "Intrinsics of the target views").  The iteration then issues sln_place_camera_step_views in the place of the pose
    launch (pose steps 0 when ``poses`` is None): beside the pose gradient it records ``intr_grad`` [iters, R, V, 4] float64 = (dL/dfx, dL/dfy,
    dL/dcx, dL/dcy) on the device, and steps the views marked ``free`` (None: all) on a float64 master: ``fx <- fx exp(-focal_step fx
    dL/dfx)``, ``fy`` likewise - with ``tie_focal`` both by the one log-scale ``-focal_step (fx dL/dfx + fy dL/dfy)`` - and ``cx <- cx -
    center_step dL/dcx``, ``cy`` likewise (``reproject.intrinsics_step_torch``).  Skew and the last row of ``K`` stay; a ``K`` with skew is
    refused.  ``start``: the ``K`` the loop begins from, as for poses.  After ``run()``: ``intrinsics()`` -> K float64,
    ``intrinsics_error(K_ref)``."""

    def __init__(self, model, rooms, bank=None, learning_rate=1e-4, noise_seed=13, image_size=256, iters=60, report=None, pictures=None,
                 retrieve=False, observed=None, mask=None, overlap_weight=0.0, overlap_rows=None, views=None, poses=None, intrinsics=None,
                 confidence=None):
        self.model, self.R, self.iters, self.lr, self.S = model, len(rooms), int(iters), float(learning_rate), int(image_size)
        dev = model.flat_params.device
        self._check_arguments(rooms, report, pictures, retrieve, observed, mask, dev, views, poses, intrinsics, confidence)      # every refusal, in front of the first launch
        if self._views is not None:      # from here on an image is b = r * V + v: observed frames and a mask tensor lose their room axis
            fold = lambda x: x.reshape(self.R * self.V, self.S, self.S) if torch.is_tensor(x) else x
            observed, mask, confidence = None if observed is None else tuple(fold(x) for x in observed), fold(mask), fold(confidence)
        self.overlap_weight = float(overlap_weight)
        self._collide_rows = check_overlap(overlap_weight, overlap_rows, [(int(rm["objs"].shape[0]), list(rm["class_names"])) for rm in rooms])
        self._bank = bank or MeshBank([n for n in set(n for rm in rooms for n in rm["class_names"]) if n not in DO_NOT_VIS and n != "__room__"], dev)
        self._retrieve, self._class_names = bool(retrieve), [list(rm["class_names"]) for rm in rooms]
        self.rows = [int(rm["objs"].shape[0]) for rm in rooms]
        self.row0 = [sum(self.rows[:r]) for r in range(self.R)]
        self.N, self.n_max = sum(self.rows), max(self.rows)
        model.eval()
        targets = self._start_rooms(rooms, noise_seed, observed, dev)
        if self._report_at is not None:
            self._report_buffers(rooms, targets, dev)
        if self._pictures_at is not None:
            self._picture_buffers(targets, dev)
        all_targets = torch.cat(targets, 0)                   # the loss of all rooms: one descriptor, per-room normalisation
        self.loss = RefineLoss(all_targets, per_room=True, valid=valid_and_labels(mask, all_targets, labels=False)[0], confidence=confidence)
        self.mask_status = self.loss.mask_status
        if self._views is not None and self.mask_status is not None:
            self.mask_status = self.mask_status.view(self.R, self.V)
        del targets, all_targets
        self._create_group(rooms, dev)
        self._head_and_placement_buffers(dev)
        self._bind_scenes(self.scenes)
        self._image_and_loss_buffers(dev)
        self._sgd_ranges()
        self.noise = torch.zeros(self.N, dtype=torch.float32, device=dev)
        self._graph, self._graph_out, self.k = GraphStep(), None, 0
        # the side stream of the wgrads / the scene backward's depth chain is PROBED for real overlap with the caller's stream, which
        # synchronises that stream: here, at set-up, not inside the first iteration's asynchronous calls (csrc/streams.hip)
        if not torch.cuda.is_current_stream_capturing():
            _lib.lib().sln_side_stream_prepare(_lib.current_stream_ptr())

    def _check_arguments(self, rooms, report, pictures, retrieve, observed, mask, dev, views=None, poses=None, intrinsics=None, confidence=None):
        """refuses what cannot run; leaves ``_report_at`` (frozenset) and ``_pictures_at`` ({iteration: slot}), None when not asked for, + "all" flags,
        ``_views`` (``check_views``: the cameras on the host, or None), ``V``, ``_poses`` (``check_poses``, or None) and ``_intr`` (``check_intrinsics``, or None)"""
        if self.R < 1:
            raise ValueError("RefineBatch needs at least one room")
        self._views = check_views(views, self.R, observed, mask, report, pictures, retrieve)
        self._poses = check_poses(poses, self._views, self.R)
        self._intr = check_intrinsics(intrinsics, self._views, self.R)
        self.V = 1 if self._views is None else int(self._views[0].shape[1])
        shape = (self.R, self.S, self.S) if self._views is None else (self.R, self.V, self.S, self.S)
        check_observed(observed, shape, dev, cuda=True, choice=retrieve)
        check_mask(mask, shape, dev, observed)
        check_confidence(confidence, shape, dev, mask, self._views)
        at, self._report_all = parse_schedule(report, self.iters, "report") or (None, False)
        self._report_at = None if at is None else frozenset(at)
        at, self._pictures_all = parse_schedule(pictures, self.iters, "pictures") or (None, False)
        self._pictures_at = None if at is None else {k: j for j, k in enumerate(at)}
        if (retrieve or report is not None) and any(len(rm["class_names"]) != int(rm["objs"].shape[0]) for rm in rooms):
            raise ValueError("class_names must name every row of a room")

    def _start_rooms(self, rooms, noise_seed, observed, dev):
        """per room: the start (``room_start``), the target scene, the target and the frozen room row -> the R targets [1, C, S, S]"""
        R, S, bank, f32 = self.R, self.S, self._bank, dict(dtype=torch.float32, device=dev)
        self.z = torch.empty(self.N, self.model.embedding_dim, **f32)
        noise = torch.zeros(max(self.iters, 1), self.N)
        # all rooms' ground-truth rows: what retrieve=True retrieves the targets' meshes for and what the report's IoU measures against
        self._gt_boxes = None
        if self._retrieve or self._report_at is not None:
            self._gt_boxes = torch.cat([rm["boxes"].detach().float() for rm in rooms]).to(dev).contiguous()
        self.target_models = self.models = self._shells = tm = None
        if self._retrieve:               # the targets' meshes from ONE retrieval launch over those rows (read back: this is set-up)
            self.target_models, self._shells = retrieve_choice(bank, self._gt_boxes, [n for nm in self._class_names for n in nm], self.rows)
            tm = self.target_models.cpu().tolist()
        self.box_last, self.angle_last = torch.empty(R, 6, **f32), torch.empty(R, **f32)
        scenes, targets, self._size_targets = [], [], []
        for r, rm in enumerate(rooms):
            a, n = self.row0[r], self.rows[r]
            # (fp32 whatever model.gemm_precision says: the refinement loop's room engines are fp32 only, and so is its starting point)
            self.z[a:a + n], noise[:self.iters, a:a + n] = room_start(self.model, rm, noise_seed, self.iters, dev, fp32=True)
            sc, tgt, sizes = room_target(rm, bank, S, tm[a:a + n] if tm is not None else None, self._shells[r] if self._shells is not None else None,
                                         observed is not None or self._views is not None)
            if self._views is not None and observed is None:
                # a room's V targets: the same ground-truth rows through each view's camera, on the single-view path (``with_view``)
                with torch.no_grad():
                    tgt = torch.cat([sc.with_view(*(x[r, v] for x in self._views)).render(rm["boxes"], rm["angles"].float())[0]
                                     for v in range(self.V)], 0)
            scenes.append(sc); targets.append(tgt); self._size_targets.append(sizes)
            self.box_last[r] = rm["boxes"][-1].detach().float(); self.angle_last[r] = rm["angles"][-1].detach().float()
        self.target_status = None
        if observed is not None:         # all targets from ONE ObservedTarget call on the batch's class tables (csrc/observed_target.hip)
            B = R * self.V
            built, status = OB.ObservedTarget(*_shared_class_tables(scenes), S, batch=B, device=dev, nch=DR.N_SCENE_CHANNELS)(*observed)
            targets, self.target_status = [built[b:b + 1] for b in range(B)], status.clone()
            if self._views is not None:
                self.target_status = self.target_status.view(R, self.V)
        self.scenes = self.target_scenes = scenes
        self.noise_all = noise.to(dev)
        return targets

    def _report_buffers(self, rooms, targets, dev):
        """report: the IoU's ground truth, the targets' full-resolution depth-hot planes (not null-filled, :332), the IoU means, ``report``"""
        R = self.R
        self._gt_angles = torch.cat([rm["angles"].detach().float() for rm in rooms]).to(dev).contiguous()
        self._visible = torch.tensor([nm not in DO_NOT_VIS for rm in rooms for nm in rm["class_names"]], dtype=torch.uint8, device=dev)
        self._target_depth = torch.cat([t[:, 41:] for t in targets], 0).contiguous()
        self._iou_mean = torch.zeros(R, dtype=torch.float64, device=dev)
        self._report_ws = torch.empty(int(_lib.lib().sln_refine_report_scratch_doubles(R)), dtype=torch.float64, device=dev)
        self.report = torch.full((max(self.iters, 1), R, 3), float("nan"), dtype=torch.float32, device=dev)

    def _picture_buffers(self, targets, dev):
        """pictures: one slot per pictured iteration, and ``target_pictures`` of the targets as built (:320: every plane written)"""
        R, S, n_pic = self.R, self.S, len(self._pictures_at)
        self._pics = SP.ScenePictures(S, batch=R, channels=DR.N_SCENE_CHANNELS, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.pictures = PictureSet(torch.zeros(n_pic, R, S, S, **u8), torch.zeros(n_pic, R, S, S, **u8), torch.zeros(n_pic, R, S, S, 3, **u8),
                                   torch.zeros(n_pic, R, dtype=torch.int32, device=dev), tuple(self._pictures_at))
        t = self._pics(torch.cat(targets, 0).contiguous())
        self.target_pictures = SP.Pictures(t.depth8.clone(), t.labels.clone(), t.rgb.clone(), None, t.status.clone())

    def _create_group(self, rooms, dev):
        """R parameter copies, R engines with their room bound, one launch program over them (``_group``)"""
        L, R, N, model, f32 = _lib.lib(), self.R, self.N, self.model, dict(dtype=torch.float32, device=dev)
        self.params = model.flat_params.detach().unsqueeze(0).repeat(R, 1).contiguous()
        self.grads = torch.zeros(R, model.flat_params.numel(), **f32)
        self._engines = model.room_engines(self.params, self.grads, self.n_max, max(int(rm["triples"].shape[0]) for rm in rooms))
        st = _lib.current_stream_ptr()
        self._keep = []
        for (h, _ws, _arr), rm in zip(self._engines, rooms):
            n = int(rm["objs"].shape[0])
            objs, tri, attrs = (rm[k].to(torch.int64).contiguous() for k in ("objs", "triples", "attributes"))
            zb, za = torch.zeros(n, model.box_dim, **f32), torch.zeros(n, dtype=torch.int64, device=dev)
            b = _lib.SlnVaeBatch()
            b.objs, b.triples, b.boxes, b.angles, b.attributes = objs.data_ptr(), tri.data_ptr(), zb.data_ptr(), za.data_ptr(), attrs.data_ptr()
            b.O, b.T = n, int(tri.shape[0])
            _lib.check(L.sln_vae_set_batch(h, C.byref(b), st), "sln_vae_set_batch")
            self._keep.append((objs, tri, attrs, zb, za))
        self.boxes_pred, self.angles_pred = torch.empty(N, model.box_dim, **f32), torch.empty(N, model.Nangle, **f32)
        self.d_boxes_pred, self.d_angles_pred = torch.zeros(N, 8, **f32), torch.empty(N, model.Nangle, **f32)
        self.dz = torch.empty(N, model.embedding_dim, **f32)
        io = _lib.SlnVaeGroupIO()
        self._row0_c = (C.c_int * R)(*self.row0)
        io.rows_total, io.row0_host = N, self._row0_c
        io.z, io.boxes_pred, io.angles_pred = self.z.data_ptr(), self.boxes_pred.data_ptr(), self.angles_pred.data_ptr()
        io.d_boxes_pred, io.d_angles_pred, io.dz = self.d_boxes_pred.data_ptr(), self.d_angles_pred.data_ptr(), self.dz.data_ptr()
        # SGD of the Linear weights / biases in the epilogue of their wgrads (one pass over the R parameter copies instead of the
        # gradient += and the optimizer's read of both and write; SLN_REFINE_SEPARATE_SGD=1: the stand-alone step over everything)
        self._step = torch.full((1,), (self.lr / 10.0) * 1.1, **f32)
        if not os.environ.get("SLN_REFINE_SEPARATE_SGD"):
            io.sgd_step = self._step.data_ptr()
        harr, g = (C.c_void_p * R)(*[e[0] for e in self._engines]), C.c_void_p()
        torch.cuda.current_stream(dev).synchronize()          # the tables of the program are uploaded with blocking copies
        _lib.check(L.sln_vae_group_create(harr, R, C.byref(io), C.byref(g)), "sln_vae_group_create")
        self._group = g

    def _head_and_placement_buffers(self, dev):
        """everything per row or per room that the head and the placement read and write, whatever the scenes (``_bind_scenes``)"""
        R, N, f32 = self.R, self.N, dict(dtype=torch.float32, device=dev)
        self.room_of_row = torch.cat([torch.full((n,), r, dtype=torch.int32) for r, n in enumerate(self.rows)]).to(dev)
        self.last_row = torch.tensor([a + n - 1 for a, n in zip(self.row0, self.rows)], dtype=torch.int32, device=dev)
        if self._report_at is not None or self._retrieve or self._collide_rows is not None:
            self._room_row = self.last_row[self.room_of_row.long()].contiguous()         # [N]: every row's room row
        self.boxes, self.idx = torch.empty(N, 6, **f32), torch.empty(N, **f32)
        self.g_boxes, self.g_idx = torch.empty(N, 6, **f32), torch.empty(N, **f32)
        self.sizes = torch.zeros(R, max(max(sc.n_vis for sc in self.scenes), 1), 3, **f32)
        self.size_loss = torch.zeros(R, **f32)
        self.g_size_loss = torch.full((1,), 2.0, **f32)               # loss = ... + 2 * size_loss (test_render_refine.py:350-352)
        # the head inside the two placement launches (SlnPlacementRoom's head fields; iteration k's noise: row k of noise_all, k a device counter)
        # (the penalty's gradient joins g_boxes / g_idx between the placement backward and the head's: the head in launches of its own)
        # (the view placement reads boxes / idx and has no head of its own: with views the head runs in launches of its own as well)
        self._fused_head = (self.n_max <= 128 and not os.environ.get("SLN_REFINE_SEPARATE_HEAD") and self._collide_rows is None
                            and self._views is None)
        self.overlap = None
        if self._collide_rows is not None:
            self._collide = torch.tensor([v for rows in self._collide_rows for v in rows], dtype=torch.uint8, device=dev)
            self.overlap = torch.zeros(max(self.iters, 1), R, dtype=torch.float64, device=dev)
            self._overlap_w64, self._overlap_w32 = torch.zeros(R, dtype=torch.float64, device=dev), torch.zeros(R, **f32)
        self._noise_step = torch.zeros(1, dtype=torch.int32, device=dev)

    def _image_and_loss_buffers(self, dev):
        """the image and its gradient, the loss outputs and the live-plane flags the loss and the scene pass share"""
        R, S, f32 = self.R, self.S, dict(dtype=torch.float32, device=dev)
        B = R * self.V                                                 # images: b = r * V + v
        self.image, self.g_image = (torch.zeros(B, DR.N_SCENE_CHANNELS, S, S, **f32) for _ in range(2))       # (planes flagged dead: never touched)
        self.loss_out = torch.empty(B, 3, **f32)
        # the semantic planes of classes without a visible pixel are zeros, and the scene pass never reads their gradients nor
        # those of such classes' depth-hot planes: the loss skips them (SlnRefineLoss::live_planes, refreshed after every scene pass)
        self.live = torch.full((B, DR.N_SCENE_CHANNELS), 3, dtype=torch.uint8, device=dev)
        self.null_mask = None
        # (only when the loss takes the flags for this geometry: below the pooled size it would read planes the sparse scene pass leaves unwritten)
        if not os.environ.get("SLN_REFINE_ALL_PLANES") and _lib.lib().sln_refine_loss_live_ok(C.byref(self.loss.desc)):
            self.loss.desc.live_planes = self.live.data_ptr()
            self.null_mask = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
            self.loss.desc.null_mask = self.null_mask.data_ptr()
            self._pooled_ones = self.loss.pooled_ones()
            self.loss.desc.pooled_ones = self._pooled_ones.data_ptr()
        self.one = torch.ones(1, **f32)
        # a room's loss is the mean of its views' (+ 2 size_loss): every image's gradient is scaled by float32(1 / V)
        self.grad_scale = self.one if self._views is None else torch.full((1,), 1.0 / self.V, **f32)
        self._view_mean = None if self._views is None else torch.empty(R, **f32)
        self.losses = torch.zeros(max(self.iters, 1), R, **f32)

    def _sgd_ranges(self):
        """what the stand-alone SGD launch steps: the decoder's parameter runs minus the tensors the wgrad launches step themselves"""
        L = _lib.lib()
        nf = int(L.sln_vae_group_fused_params(self._group, None, None, 0))
        ptrs, lens = (C.c_void_p * nf)(), (C.c_int64 * nf)()
        if nf > 0:
            L.sln_vae_group_fused_params(self._group, ptrs, lens, nf)
        base = self.params.data_ptr()
        rg = cut_ranges(self.model.decoder_param_ranges(), [(int(ptrs[i]) - base) // 4 for i in range(nf)], [int(lens[i]) for i in range(nf)])
        self._sgd_off = (C.c_int64 * len(rg))(*[a for a, _ in rg])
        self._sgd_len = (C.c_int64 * len(rg))(*[b for _, b in rg])
        self._n_rg = len(rg)

    def _bind_scenes(self, scenes):
        """Everything of the launch program that follows the rooms' SCENES (their models' vertices and face lists): the padded face
        buffers, the class table of the faces, the placement table and the scene pass's workspace.  Called at construction with the
        target scenes and, with retrieve=True, once more by the first ``run()`` with the scenes of the iterates' meshes (which may
        change F2); the size targets, the head's buffers and everything per row stay where they are."""
        R, V, N, na, dev = self.R, self.V, self.N, self.model.Nangle, self.boxes.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.scenes = scenes
        self.chan, self.dch = _shared_class_tables(scenes)
        self.F2 = 2 * max(sc.desc.F for sc in scenes)
        # (with views: image b = r * V + v; a room's table entry points at its view 0, view v lies 9 * F2 floats behind it)
        self.faces = torch.zeros(R * V, self.F2, 3, 3, **f32)         # rows beyond a room's 2 F stay degenerate triangles of no class
        self.g_faces = torch.empty(R * V, self.F2, 3, 3, **f32)
        self.cls = cls = torch.full((R * V, self.F2), -1, dtype=torch.int32, device=dev)
        tab = (_lib.SlnPlacementRoom * R)()
        for r, sc in enumerate(scenes):
            cls[r * V:(r + 1) * V, :2 * sc.desc.F] = sc.cls2[0]
            e, a = tab[r], self.row0[r]
            e.P = sc.desc
            e.boxes, e.angles = self.boxes.data_ptr() + 24 * a, self.idx.data_ptr() + 4 * a
            e.size_target = self._size_targets[r].data_ptr() if sc.n_vis else None
            e.faces_out, e.sizes, e.size_loss = self.faces[r * V].data_ptr(), self.sizes[r].data_ptr(), self.size_loss.data_ptr() + 4 * r
            e.grad_faces, e.grad_size_loss = self.g_faces[r * V].data_ptr(), self.g_size_loss.data_ptr()
            e.grad_boxes, e.grad_angles = self.g_boxes.data_ptr() + 24 * a, self.g_idx.data_ptr() + 4 * a
            if self._fused_head:
                e.boxes_pred, e.angles_pred = self.boxes_pred.data_ptr() + 24 * a, self.angles_pred.data_ptr() + 4 * na * a
                e.noise, e.noise_step, e.noise_stride = self.noise_all.data_ptr() + 4 * a, self._noise_step.data_ptr(), N
                e.box_last, e.angle_last = self.box_last.data_ptr() + 24 * r, self.angle_last.data_ptr() + 4 * r
                e.grad_boxes_pred, e.grad_angles_pred = self.d_boxes_pred.data_ptr() + 32 * a, self.d_angles_pred.data_ptr() + 4 * na * a
                e.n_angle, e.ld_gb, e.beta = na, 8, 2.0
        self._place_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
        if self._views is not None and getattr(self, "_cams", None) is None:
            # the camera table [R * V] of SlnPlacementCamera (K[9], R[9], t[3]), uploaded once
            self._cams = torch.cat([x.reshape(R * V, -1) for x in self._views], 1).contiguous().to(dev)
            if self._poses is not None or self._intr is not None:
                self._pose_buffers(dev)
            if self._intr is not None:
                self._intr_buffers(dev)
        self.scene_ws = torch.empty(int(_lib.lib().sln_scene_workspace_bytes(R * V, self.F2, self.S)), dtype=torch.uint8, device=dev)

    def _pose_buffers(self, dev):
        """poses: the loop's starting cameras in the table, the float64 master [R * V, 12] = double(float32 entry) (R row-major, then t), the
        free flags and the record of the gradients"""
        R, V, ps = self.R, self.V, self._poses or dict(start=None, free=None)      # (intrinsics alone: the poses are held, their steps 0)
        if ps["start"] is not None:
            self._cams[:, 9:] = torch.cat([x.reshape(R * V, -1) for x in ps["start"]], 1).to(dev)
        self._pose = self._cams[:, 9:].double().contiguous()
        self._pose_free = None if ps["free"] is None else ps["free"].reshape(-1).to(torch.uint8).to(dev).contiguous()
        self.pose_grad = torch.zeros(max(self.iters, 1), R, V, 6, dtype=torch.float64, device=dev)

    def _intr_buffers(self, dev):
        """intrinsics: the loop's starting K in the table, the float64 master [R * V, 4] = double(float32 entry) (fx, fy, cx, cy), the free
        flags and the record of the gradients"""
        R, V, it = self.R, self.V, self._intr
        if it["start"] is not None:
            self._cams[:, :9] = it["start"].reshape(R * V, 9).to(dev)
        self._intr_master = self._cams[:, [0, 4, 2, 5]].double().contiguous()
        self._intr_free = None if it["free"] is None else it["free"].reshape(-1).to(torch.uint8).to(dev).contiguous()
        self.intr_grad = torch.zeros(max(self.iters, 1), R, V, 4, dtype=torch.float64, device=dev)

    def intrinsics(self):
        """K [R, V, 3, 3] float64: the master copy of the refined focal lengths and principal points in the views' K, whose other entries
        are the table's (needs ``intrinsics=``)"""
        if self._intr is None:
            raise ValueError("no intrinsics are refined: RefineBatch(views=, intrinsics=)")
        K = self._cams[:, :9].double()
        K[:, [0, 4, 2, 5]] = self._intr_master
        return K.view(self.R, self.V, 3, 3)

    def intrinsics_error(self, K_ref):
        """``reproject.intrinsics_error`` of the refined K against a reference K [R, V, 3, 3] -> (relative focal error [R, V], distance of the
        principal points in pixels [R, V]) float64 on the device"""
        K = self.intrinsics()
        return RP.intrinsics_error(K, torch.as_tensor(K_ref).to(K.device))

    def poses(self):
        """(Rm [R, V, 3, 3], t [R, V, 3]) float64: the master copy of the refined poses (needs ``poses=``; with ``intrinsics=`` alone the poses
        the loop holds)"""
        if self._poses is None and self._intr is None:
            raise ValueError("no poses are refined: RefineBatch(views=, poses=)")
        m = self._pose.view(self.R, self.V, 12)
        return m[..., :9].reshape(self.R, self.V, 3, 3).clone(), m[..., 9:].clone()

    def pose_error(self, Rm_ref, t_ref):
        """``reproject.pose_error`` of the refined poses against reference poses [R, V, 3, 3], [R, V, 3] -> (angle [R, V] in radians, distance
        of the camera centres [R, V]) float64 on the poses' device"""
        Rm, t = self.poses()
        return RP.pose_error(Rm, t, torch.as_tensor(Rm_ref).to(Rm.device), torch.as_tensor(t_ref).to(Rm.device))

    def _retrieve_iterates(self):
        """retrieve=True: the iterates' meshes are those retrieved for the FIRST iterate's boxes (testing/test_render_refine.py:324-326:
        ``model_infos`` is what the first ``mesh_render_func`` call on ``boxes_pred`` returns) - one launch over ``self.boxes`` behind
        ``_first_iterate_sizes``' forward, read back (set-up, outside any capture), frozen from then on.  The room rows are the ground
        truth's, so the shells stay the targets'."""
        table = self._bank.table
        index = {n: k for k, n in reversed(list(enumerate(table.vocab)))}
        cls = torch.tensor([index.get(n, -1) for nm in self._class_names for n in nm], dtype=torch.int32, device=self.boxes.device)
        self.models = RT.retrieve_models(self.boxes, cls, self._room_row, table)
        host = self.models.cpu().tolist()
        if host == self.target_models.cpu().tolist():
            return
        self._bind_scenes([RefineScene(names, self._bank, sc.room, self.S, models=host[a:a + n], shell=sc.shell)
                           for names, sc, a, n in zip(self._class_names, self.target_scenes, self.row0, self.rows)])

    def model_ids(self, target=False):
        """[[id per row, None where nothing is retrieved (room rows, classes without a model)] per room] of the iterates' meshes
        (``target=True``: the targets'); needs retrieve=True and, for the iterates, the first ``run()``"""
        models = self.target_models if target else self.models
        if models is None:
            raise ValueError("no retrieval yet: RefineBatch(retrieve=True), and run() for the iterates' meshes")
        table, host = self._bank.table, models.cpu().tolist()
        return [[table.id_of(table.vocab.index(n), host[a + i]) if host[a + i] >= 0 else None for i, n in enumerate(names)]
                for names, a in zip(self._class_names, self.row0)]

    def _forward_to_placement(self, noise):
        """decoder of all rooms, the head (``noise`` [N]; its own launch unless the placement launch holds it) and the placement"""
        L, st, P = _lib.lib(), _lib.current_stream_ptr(), _lib.ptr
        _lib.check(L.sln_vae_group_decoder(self._group, st), "sln_vae_group_decoder")
        if not self._fused_head:
            _lib.check(L.sln_refine_head_forward_rooms(self.N, self.model.Nangle, P(self.room_of_row), P(self.last_row), P(self.boxes_pred),
                                                       P(self.angles_pred), P(noise), P(self.box_last), P(self.angle_last), 2.0, P(self.boxes),
                                                       P(self.idx), st), "sln_refine_head_forward_rooms")
        if self._views is not None:
            _lib.check(L.sln_place_forward_views(P(self._place_tab), P(self._cams), self.R, self.V, self.F2 // 2, 9 * self.F2, st), "sln_place_forward_views")
        else:
            _lib.check(L.sln_place_forward_rooms(P(self._place_tab), self.R, self.F2 // 2, st), "sln_place_forward_rooms")

    def _first_iterate_sizes(self):
        """The size penalty holds every object to the size of the FIRST iterate (testing/test_render_refine.py:319-327: ``size_infos`` is
        what the first ``mesh_render_func`` call on ``boxes_pred`` returns; the sizes of the target render are ``unused_sizes``): one
        decoder + head + placement forward of all rooms with iteration 0's z, parameters and noise row, whose ``sizes`` become the
        rooms' targets.  Iteration 0 then measures its own sizes against themselves: a size loss of exactly 0 with zero gradient - the
        reference's ``size_loss = 0.0`` of a first call.  Run by ``run()`` in front of iteration 0 (eagerly, outside any capture), so
        that edits of ``z`` or ``params`` between construction and the first ``run()`` are the first iterate's; frozen from then on."""
        self._forward_to_placement(self.noise_all[0])
        for r, sc in enumerate(self.scenes):
            if sc.n_vis:
                self._size_targets[r].copy_(self.sizes[r, :sc.n_vis])

    def launches(self):
        f, b, s1 = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().sln_vae_group_launches(self._group, C.byref(f), C.byref(b), C.byref(s1)), "sln_vae_group_launches")
        return dict(decoder_forward=f.value, decoder_backward=b.value, single_room_fallbacks=s1.value)

    def _iteration(self, noise, out, report_out=None, pictures_out=None, overlap_out=None, pose_out=None, intr_out=None):
        """one iteration of every room on the current stream; ``noise`` [N], ``out`` [R] receives the rooms' losses, ``report_out``
        [R, 3] (a reported iteration) the report, ``pictures_out`` (a pictured iteration) = (depth8, labels, rgb, status) of one slot,
        ``overlap_out`` [R] float64 (with the penalty on) the rooms' unweighted penalties, ``pose_out`` [R, V, 6] float64 (with ``poses``) the
        gradients of the views' poses, ``intr_out`` [R, V, 4] float64 (with ``intrinsics``, then together with ``pose_out``) those of their intrinsics"""
        L, st, P = _lib.lib(), _lib.current_stream_ptr(), _lib.ptr
        N, R, na, S, B = self.N, self.R, self.model.Nangle, self.S, self.R * self.V
        self._forward_to_placement(noise)
        if report_out is not None:      # (the fused head lives in the placement launch: boxes / idx of this iterate exist from here on)
            _lib.check(L.sln_layout_cuboid_iou(P(self.boxes), P(self.idx), P(self._gt_boxes), P(self._gt_angles), P(self._room_row), P(self._visible),
                                               P(self.room_of_row), R, 1, N, None, P(self._iou_mean), st), "sln_layout_cuboid_iou")
        rl = self.loss
        live = (P(self.live), P(self.null_mask)) if rl.desc.live_planes else ()        # the scene pass refreshes the live-plane flags
        forward = L.sln_scene_forward_live if live else L.sln_scene_forward
        _lib.check(forward(P(self.faces), P(self.cls), B, self.F2, S, self.chan.numel(), P(self.chan), P(self.dch), 0.1, 0.001, 100.0, 1e-3,
                           P(self.scene_ws), P(self.image), *live, st), "sln_scene_forward_live" if live else "sln_scene_forward")
        _lib.check(L.sln_refine_loss_forward(rl.desc, P(self.image), P(rl.target_depth), P(rl.labels), P(rl.inv_count), P(rl.ws), P(self.loss_out), st),
                   "sln_refine_loss_forward")
        if self._views is not None:     # a room's loss: the mean of its views' losses (exact for V = 1)
            torch.mean(self.loss_out[:, 0].view(R, self.V), 1, out=self._view_mean)
            torch.add(self._view_mean, self.size_loss, alpha=2.0, out=out)
        else:
            torch.add(self.loss_out[:, 0], self.size_loss, alpha=2.0, out=out)
        if report_out is not None:      # reads the image and the loss forward's partial sums, consumes (and re-arms) the IoU means
            _lib.check(L.sln_refine_report(rl.desc, P(self.image), P(self._target_depth), P(rl.ws), P(self._report_ws), P(self._iou_mean), P(report_out),
                                           st), "sln_refine_report")
        if pictures_out is not None:    # the iterate as the loss saw it: the planes `live` flags dead are not read
            self._pics.into(self.image, self.live, *pictures_out[:3], None, pictures_out[3])
        _lib.check(L.sln_refine_loss_backward(rl.desc, P(rl.ws), P(self.grad_scale), P(self.g_image), st), "sln_refine_loss_backward")
        _lib.check(L.sln_scene_backward(P(self.faces), P(self.cls), B, self.F2, S, self.chan.numel(), P(self.chan), P(self.dch), 1e-3, P(self.scene_ws),
                                        P(self.g_image), P(self.g_faces), st), "sln_scene_backward")
        if self._views is not None:     # the views' adjoints meet in world space: one launch, one writer per row
            _lib.check(L.sln_place_backward_views(P(self._place_tab), P(self._cams), R, self.V, self.n_max, 9 * self.F2, st), "sln_place_backward_views")
            if intr_out is not None:    # in the pose launch's place: ONE launch steps pose and K, both from the gradients of the old camera
                ps, it = self._poses or dict(rot_step=0.0, trans_step=0.0), self._intr
                _lib.check(L.sln_place_camera_step_views(P(self._place_tab), P(self._cams), P(self._pose), P(pose_out), P(self._pose_free),
                                                         P(self._intr_master), P(intr_out), P(self._intr_free), R, self.V, 9 * self.F2, ps["rot_step"],
                                                         ps["trans_step"], it["focal_step"], it["center_step"], int(it["tie_focal"]), st),
                           "sln_place_camera_step_views")
            elif pose_out is not None:  # behind the placement's backward, which still reads the old cameras: the table is stepped in place
                _lib.check(L.sln_place_pose_step_views(P(self._place_tab), P(self._cams), P(self._pose), P(pose_out), P(self._pose_free), R, self.V,
                                                       9 * self.F2, self._poses["rot_step"], self._poses["trans_step"], st), "sln_place_pose_step_views")
        else:
            _lib.check(L.sln_place_backward_rooms(P(self._place_tab), R, self.n_max, st), "sln_place_backward_rooms")
        if overlap_out is not None:
            # all rooms' rows as ONE layout of R rooms; += onto the gradients the placement backward has just written (every row of every room,
            # zeros for rows without a visible object: csrc/placement.hip place_backward_body), in front of the head's backward and its two hooks
            _lib.check(L.sln_layout_overlap_penalty(P(self.boxes), P(self.idx), P(self._room_row), P(self._collide), P(self.room_of_row), R, 1, N,
                                                    self.overlap_weight, 1, P(overlap_out), P(self.g_boxes), P(self.g_idx), st),
                       "sln_layout_overlap_penalty")
            torch.mul(overlap_out, self.overlap_weight, out=self._overlap_w64)            # loss = ... + 2 size_loss + float32(weight * penalty)
            self._overlap_w32.copy_(self._overlap_w64)
            out.add_(self._overlap_w32)
        if not self._fused_head:
            _lib.check(L.sln_refine_head_backward_rooms(N, na, P(self.room_of_row), P(self.last_row), P(self.angles_pred), P(self.g_boxes), P(self.g_idx),
                                                        2.0, P(self.d_boxes_pred), 8, P(self.d_angles_pred), st), "sln_refine_head_backward_rooms")
        _lib.check(L.sln_vae_group_decoder_backward(self._group, st), "sln_vae_group_decoder_backward")
        _lib.check(L.sln_refine_sgd_rooms(P(self.params), P(self.grads), R, self.params.shape[1], self._sgd_off, self._sgd_len, self._n_rg,
                                          (self.lr / 10.0) * 1.1, P(self.z), P(self.dz), self.z.numel(), 2e-4 * 1.1, st), "sln_refine_sgd_rooms")

    def run(self, iters=None, capture=False):
        """``iters`` more iterations (default: all that remain).  ``capture``: one iteration recorded into a hipGraph and replayed -
        a LINEAR graph: inside a capture the library keeps its side work (wgrads, the depth chain of the scene backward) on the
        captured stream, because this runtime replays forked graphs node by node from the host without overlapping the branches.
        What a replay buys is the host (0.09 ms of enqueue per iteration instead of 0.3-0.4 ms); the GPU time is that of the one-stream
        order, ~5 % above the eager loop with its side streams (16 rooms: 1.66 against 1.56-1.59 ms) - eager is the default."""
        n = (self.iters - self.k) if iters is None else int(iters)
        if self.k + n > self.iters:
            raise ValueError("RefineBatch was built for %d iterations (the noise of every iteration is drawn at construction)" % self.iters)
        for name, at, is_all in (("report", self._report_at, self._report_all), ("pictures", self._pictures_at, self._pictures_all)):
            if capture and at is not None and not is_all:
                raise ValueError("run(capture=True) replays one graph for every iteration: %s must be 'all' or None" % name)
        camera = self._poses is not None or self._intr is not None        # a camera step is issued: pose_grad is recorded
        if capture and self._graph_out is None:       # what the graph writes: copied to the iteration's own rows after every captured step
            self._graph_out = (self.loss_out.new_empty(self.R), self.loss_out.new_empty(self.R, 3) if self._report_all else None,
                               tuple(torch.empty_like(t[0]) for t in self.pictures[:4]) if self._pictures_all else None,
                               torch.empty_like(self.overlap[0]) if self.overlap is not None else None,
                               torch.empty_like(self.pose_grad[0]) if camera else None,
                               torch.empty_like(self.intr_grad[0]) if self._intr is not None else None)
        if n > 0 and self.k == 0:
            self._first_iterate_sizes()
            if self._retrieve and self.models is None:
                self._retrieve_iterates()
        step = lambda: self._iteration(self.noise, *self._graph_out)
        for _ in range(n):
            k = self.k
            rep = self.report[k] if self._report_at is not None and k in self._report_at else None
            slot = None if self._pictures_at is None else self._pictures_at.get(k)
            pic = None if slot is None else tuple(t[slot] for t in self.pictures[:4])
            if capture:
                if not self._fused_head:
                    self.noise.copy_(self.noise_all[k])
                self._graph.run(step)
                self.losses[k].copy_(self._graph_out[0])
                if rep is not None:
                    rep.copy_(self._graph_out[1])
                for dst, src in zip(pic or (), self._graph_out[2] or ()):
                    dst.copy_(src)
                if self.overlap is not None:
                    self.overlap[k].copy_(self._graph_out[3])
                if camera:
                    self.pose_grad[k].copy_(self._graph_out[4])
                if self._intr is not None:
                    self.intr_grad[k].copy_(self._graph_out[5])
            else:
                self._iteration(self.noise_all[k], self.losses[k], rep, pic, self.overlap[k] if self.overlap is not None else None,
                                self.pose_grad[k] if camera else None, self.intr_grad[k] if self._intr is not None else None)
            self.k += 1
        return self.losses[:self.k]

    def results(self):
        """[(boxes_full [n,6], angle idx [n]) per room] of the last iteration"""
        return [(self.boxes[a:a + n], self.idx[a:a + n]) for a, n in zip(self.row0, self.rows)]

    def close(self):
        L = _lib.lib()
        if getattr(self, "_group", None) is not None:
            torch.cuda.synchronize()
            L.sln_vae_group_destroy(self._group)
            self._group = None
        for e in getattr(self, "_engines", []):
            L.sln_vae_destroy(e[0])
        self._engines = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def finetune_vae_fast_batch(model, rooms, iters=60, bank=None, learning_rate=1e-4, noise_seed=13, image_size=256, capture=False, report=None,
                            pictures=None, retrieve=False, observed=None, mask=None, overlap_weight=0.0, overlap_rows=None, views=None, poses=None,
                            intrinsics=None, confidence=None):
    """``finetune_vae_fast`` for R rooms at once (see ``RefineBatch``): every room from ``model``'s parameters, its own z, its own
    noise stream (seeded like a single-room call).  -> (losses [iters, R] on the device, [(boxes, angle idx) per room]) and, only when
    ``report`` is given, the report [iters, R, 3] as a further element; only when ``pictures`` is given, the pair
    (``RefineBatch.pictures``, ``RefineBatch.target_pictures``) as the last one.  ``observed`` / ``mask`` / ``confidence`` / ``overlap_weight`` /
    ``overlap_rows`` / ``views``: as ``RefineBatch``'s (``views`` combines with neither ``report``, ``pictures`` nor ``retrieve=True``).  ``poses``: as
    ``RefineBatch``'s; only when it is given, the pair (``RefineBatch.poses()``, ``RefineBatch.pose_grad``) is a further element.
    ``intrinsics``: as ``RefineBatch``'s; only when it is given, the pair (``RefineBatch.intrinsics()``, ``RefineBatch.intr_grad``) is the last one."""
    rb = RefineBatch(model, rooms, bank=bank, learning_rate=learning_rate, noise_seed=noise_seed, image_size=image_size, iters=iters, report=report,
                     pictures=pictures, retrieve=retrieve, observed=observed, mask=mask, overlap_weight=overlap_weight, overlap_rows=overlap_rows,
                     views=views, poses=poses, intrinsics=intrinsics, confidence=confidence)
    try:
        out = (rb.run(capture=capture).clone(), [(b.clone(), i.clone()) for b, i in rb.results()])
        if report is not None:
            out += (rb.report.clone(),)
        if pictures is not None:
            out += ((rb.pictures, rb.target_pictures),)             # (buffers of their own: nothing of the batch's is referenced)
        if poses is not None:
            out += ((rb.poses(), rb.pose_grad.clone()),)
        if intrinsics is not None:
            out += ((rb.intrinsics(), rb.intr_grad.clone()),)
    finally:
        rb.close()
    return out


def finetune_vae(model, objs, triples, boxes_gt, angles_gt, attributes, class_names, iters=60, render_fn=None, bank=None,
                 learning_rate=1e-4, noise_seed=13, image_size=256, log=None, observed=None, mask=None, overlap_weight=0.0, overlap_rows=None,
                 views=None, poses=None, intrinsics=None, confidence=None):
    """finetune_VAE's inner loop for ONE room (test_render_refine.py:265-359) on synthetic meshes.
    ``observed`` / ``mask``: as ``finetune_vae_fast``'s, on the boxes' device whichever it is - the target from ``observed_target_torch`` on
    the room's class tables, the loss from ``refinement_loss_masked``.  ``overlap_weight`` / ``overlap_rows``: as ``finetune_vae_fast``'s (on CPU
    tensors the penalty is ``evaluate.overlap_penalty_torch``).  ``confidence``: as ``finetune_vae_fast``'s (``[V, S, S]`` with ``views``), the
    loss from ``refinement_loss_confidence`` - the autograd yardstick of the confidence kernels' loop.
    ``views``: None, or ``(K [V, 3, 3], Rm [V, 3, 3], t [V, 3])`` - ``RefineBatch``'s ``views`` for one room, in autograd: every view is
    rendered with ``render_fn(..., camera=(K, Rm, t))``, the loss is ``mean_v L_v + 2 size_loss`` with ``L_v`` the view's depth and semantic
    terms over its own image; ``observed`` and a tensor ``mask`` are then ``[V, S, S]``.  The yardstick of the view kernels' loop.
    ``poses``: None, or ``RefineBatch``'s ``poses`` for one room (``free`` [V], ``start`` (Rm [V, 3, 3], t [V, 3])), in autograd: per view the
    pose is a leaf ``(omega, tau)`` at 0, the world vertices are moved to ``E (Rm v + t) + tau`` in torch (``E = I + [omega]x + [omega]x^2 / 2``:
    ``exp`` to the order the gradient at 0 needs) in front of ``render_fn(..., camera=(K, I, 0))``, the leaf is stepped by ``RefineBatch``'s
    rule and folded into the float64 ``(Rm, t)`` with ``reproject.pose_step_torch`` after every iteration; the view's camera is the float32
    rounding of that pair.  The yardstick of sln_place_pose_step_views inside the loop.
    ``intrinsics``: None, or ``RefineBatch``'s ``intrinsics`` for one room (``free`` [V], ``start`` K [V, 3, 3]), in autograd: per view a leaf
    ``(sx, sy, dcx, dcy)`` at 0; the camera-space vertices are moved in torch to ``x' = e^sx x + dcx (z + proj_eps) / fx``, ``y' = e^sy y + dcy
    (z + proj_eps) / fy`` in front of ``render_fn(..., camera=(K, I, 0))``, so that the unchanged ``K`` (zero skew) projects them where
    ``K`` with ``fx e^sx, fy e^sy, cx + dcx, cy + dcy`` would; the leaf's gradient is ``(fx dL/dfx, fy dL/dfy, dL/dcx, dL/dcy)``, stepped by
    ``RefineBatch``'s rule and folded into the float64 ``K`` with ``reproject.intrinsics_step_torch`` after every iteration; the view's ``K``
    is the float32 rounding of it.  Composes with the pose leaf.  The yardstick of sln_place_camera_step_views inside the loop.
    Returns the list of per-iteration losses and the final (boxes_pred, angles_idx); with ``poses``, the final ``(Rm [V, 3, 3], t [V, 3])``
    float64 as a further element; with ``intrinsics``, the final ``K [V, 3, 3]`` float64 as the last one."""
    render_fn, dev = render_fn or DR.scene_render, boxes_gt.device
    cams = check_views(views, None, observed, mask)
    pose = check_poses(poses, cams)
    intr = check_intrinsics(intrinsics, cams)
    if cams is None:
        observed, mask = _one_room_arguments(observed, mask, int(image_size), dev, False, bank)
        confidence = _one_room_confidence(confidence, mask, int(image_size), dev)
    else:
        cams = [tuple(x[0, v] for x in cams) for v in range(int(cams[0].shape[1]))]
        shape = (len(cams), int(image_size), int(image_size))
        check_observed(observed, shape, dev, False, choice=bank is not None and bank.has_choice())
        check_mask(mask, shape, dev, observed)
        check_confidence(confidence, shape, dev, mask, cams)
    overlap = _one_room_overlap(overlap_weight, overlap_rows, class_names, int(boxes_gt.shape[0]), dev)
    bank = bank or MeshBank([n for n in set(class_names) if n not in DO_NOT_VIS], dev)
    model.eval()
    # (the noise rows: one randn(n) per iteration behind the z draw, which is the stream the reference draws inside its loop, :304)
    z, noise_rows = room_start(model, dict(objs=objs, triples=triples, boxes=boxes_gt, angles=angles_gt, attributes=attributes), noise_seed, iters, dev)
    z.requires_grad_(True)
    room_box = boxes_gt[-1].detach().clone()
    # target: the meshes retrieved for the ground truth (test_render_refine.py:319); iterates: those of iteration 0's boxes (:324-326)
    choose, models_gt, models_it, shell = bank.has_choice(), None, None, None
    if choose:
        models_gt, shells = retrieve_choice(bank, boxes_gt, class_names)
        models_gt, shell = models_gt.cpu().tolist(), (shells[0] if shells is not None else None)
    v, f, ranges, sizes, _ = assemble_scene(boxes_gt, angles_gt.float(), class_names, bank, room_box, models=models_gt, shell=shell)
    with torch.no_grad():
        if observed is None and cams is not None:
            target = torch.cat([render_fn(v, f, ranges, room_box, image_size=image_size, camera=cam) for cam in cams], 0)
        elif observed is None:
            target = render_fn(v, f, ranges, room_box, image_size=image_size)
        else:
            _, chan, dch = DR.class_tables(ranges.keys())
            target, _ = OB.observed_target_torch(observed[0], observed[1], chan, dch, nch=DR.N_SCENE_CHANNELS)
    valid, labels = valid_and_labels(mask, target)
    conf = None
    if confidence is not None:
        conf, labels = confidence_and_labels(confidence, target)
    if pose is not None:                 # the float64 pair the loop steps; K stays the view's
        pose_R, pose_t = (x[0].double() for x in (pose["start"] if pose["start"] is not None else (torch.stack([c[1] for c in cams])[None],
                                                                                                     torch.stack([c[2] for c in cams])[None])))
        pose_free = [True] * len(cams) if pose["free"] is None else pose["free"][0].tolist()
    if intr is not None:                 # the float64 K the loop steps
        intr_K = (intr["start"][0] if intr["start"] is not None else torch.stack([c[0] for c in cams])).double()
        intr_free = [True] * len(cams) if intr["free"] is None else intr["free"][0].tolist()
    if pose is not None or intr is not None:
        eye3 = torch.eye(3, dtype=torch.float32, device=dev)
    size_target = None                   # the sizes of the FIRST iterate (:319-327: size_infos), not the target's (its sizes are "unused_sizes")
    losses = []
    for k in range(iters):
        opt = torch.optim.SGD([{'params': [z]}, {'params': list(model.parameters()), 'lr': learning_rate / 10.0}], lr=2e-4,
                              nesterov=True, momentum=0.1)
        boxes_pred, angles_pred = model.decoder(z, objs, triples, attributes)
        boxes_pred.register_hook(fix_grad)
        boxes_pred = torch.cat([boxes_pred[:-1], boxes_gt[-1:]], 0)
        idx = softargmax(angles_pred, sum_dim=1) + noise_rows[k].to(dev) / 10.0
        idx.register_hook(quad_grad)
        idx = torch.cat([idx[:-1], angles_gt[-1:].float()], 0)
        if choose and models_it is None:
            models_it = retrieve_choice(bank, boxes_pred, class_names)[0].cpu().tolist()
        v, f, ranges, sizes_k, size_loss = assemble_scene(boxes_pred, idx, class_names, bank, room_box, size_target, models=models_it, shell=shell)
        if size_target is None:
            size_target = [s.clone() for s in sizes_k]
        if cams is not None:            # mean over the views of each view's own loss, the size loss once
            per_view, leaves, intr_leaves = [], [], []
            for vi, cam in enumerate(cams):
                if pose is not None or intr is not None:    # the view's camera applied in torch, the leaves' motions behind it, an identity pose for the render
                    Rm32, t32 = (pose_R[vi].float().to(dev), pose_t[vi].float().to(dev)) if pose is not None else (cam[1].to(dev), cam[2].to(dev))
                    moved, K32 = torch.matmul(v, Rm32.t()) + t32, cam[0]
                    if pose is not None:
                        om, ta = (torch.zeros(3, dtype=torch.float32, device=dev, requires_grad=True) for _ in range(2))
                        leaves.append((om, ta))
                        W = RP._skew(om)
                        E = eye3 + W + torch.matmul(W, W) / 2.0
                        moved = torch.matmul(moved, E.t()) + ta
                    if intr is not None:
                        sc = torch.zeros(4, dtype=torch.float32, device=dev, requires_grad=True)
                        intr_leaves.append(sc)
                        K32 = intr_K[vi].float()
                        moved = RP.intrinsics_move(moved, sc, float(K32[0, 0]), float(K32[1, 1]))
                    image = render_fn(moved, f, ranges, room_box, image_size=image_size, camera=(K32, eye3, torch.zeros(3)))
                else:
                    image = render_fn(v, f, ranges, room_box, image_size=image_size, camera=cam)
                tgt, lab = target[vi:vi + 1], [t[vi:vi + 1] for t in labels]
                if conf is not None:
                    per_view.append(refinement_loss_confidence(image, tgt, lab, 0.0, conf[vi:vi + 1]))
                elif valid is not None:
                    per_view.append(refinement_loss_masked(image, tgt, lab, 0.0, valid[vi:vi + 1]))
                else:
                    per_view.append(refinement_loss(image, tgt, lab, 0.0))
            loss, dl, sl = (torch.stack([p[j] for p in per_view]).mean() for j in range(3))
            loss = loss + size_loss * 2.0
        else:
            image = render_fn(v, f, ranges, room_box, image_size=image_size)
            if conf is not None:
                loss, dl, sl = refinement_loss_confidence(image, target, labels, size_loss, conf)
            elif valid is not None:
                loss, dl, sl = refinement_loss_masked(image, target, labels, size_loss, valid)
            else:
                loss, dl, sl = refinement_loss(image, target, labels, size_loss)
        if overlap is not None:
            loss = loss + _overlap_term(boxes_pred, idx, overlap, overlap_weight)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if pose is not None:
            for vi, (om, ta) in enumerate(leaves):
                if pose_free[vi] and (pose["rot_step"] != 0.0 or pose["trans_step"] != 0.0):
                    pose_R[vi], pose_t[vi] = RP.pose_step_torch(pose_R[vi], pose_t[vi], -pose["rot_step"] * om.grad.double().cpu(),
                                                                -pose["trans_step"] * ta.grad.double().cpu())
        if intr is not None:
            for vi, sc in enumerate(intr_leaves):
                if intr_free[vi] and (intr["focal_step"] != 0.0 or intr["center_step"] != 0.0):
                    g, K32 = sc.grad.double().cpu(), intr_K[vi].float().double()
                    grad = torch.stack((g[0] / K32[0, 0], g[1] / K32[1, 1], g[2], g[3]))
                    intr_K[vi] = RP.intrinsics_step_torch(intr_K[vi], grad, intr["focal_step"], intr["center_step"], intr["tie_focal"])
        if hasattr(model, "params_changed"):
            model.params_changed()
        losses.append(float(loss.detach()))
        if log:
            log("iter %d: loss %.4f (depth %.4f, semantic %.4f)" % (k, losses[-1], float(dl), float(sl)))
    out = (losses, (boxes_pred.detach(), idx.detach()))
    if pose is not None:
        out += ((pose_R, pose_t),)
    if intr is not None:
        out += (intr_K,)
    return out
