"""Mesh retrieval: counterpart of ``models/misc.py`` ``suncg_retrieve`` (:34-64), ``wall_retrieve`` (:123-137) and ``floor_retrieve``
(:139-152).  For every object the reference picks, among all models of the object's class, the one whose bounding-box edge ratios
``(y/x, z/x)`` are nearest (L1) to those of the predicted box - a python loop per object and model.  Here the choice is one launch over
all rows of all rooms (and of S layouts of them): ``csrc/mesh_retrieve.hip``.

What the choice needs is the ``{id, bbox_min, bbox_max}`` table only (``suncg_data_many.json``); no mesh is read.  The output is an
argmin, so kernel and restatement follow the reference operation by operation:

  float32   the six box entries times the room row's [3], [4], [5] (one multiplication each, :36-42), the three differences (:50-52),
            the quotients dy/dx, dz/dx (:53);
  float64   ``|t0 - r0| + |t1 - r1|`` against the table's ratios (:58-60), which are formed on the host in float64;
  np.argmin the first minimum wins; a NaN distance beats everything and the first NaN is kept.

``retrieve_models`` / ``retrieve_shell`` call the kernels (device tensors; a missing library is an error), ``retrieve_models_torch`` /
``retrieve_shell_torch`` are the same in torch ops on any device: what the tests and tools/retrieve_time.py hold the kernels to.
``suncg_retrieve`` / ``wall_retrieve`` / ``floor_retrieve`` keep the reference's call shapes over tables set with ``configure``.
"""
import numpy as np
import torch

from .. import _lib


def _ratios(lo, hi):
    """(size_y / size_x, size_z / size_x) in float64, as :58-59 form them"""
    size = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([size[1] / size[0], size[2] / size[0]], dtype=np.float64)


class ModelTable:
    """The model table as the kernel reads it.  ``data``: {class name: [{"id", "bbox_min", "bbox_max"}, ...]} (the shape of
    suncg_data_many.json), ``vocab``: ``object_idx_to_name`` - the class index of a row (``objs``) indexes it; a class of the
    vocabulary without an entry in ``data`` has no models.  ``class_ptr`` [len(vocab) + 1] int32 and ``ratio`` [M, 2] float64 live on
    ``device``, ``ids[c]`` (the id strings of class c, table order) on the host."""

    def __init__(self, data, vocab, device="cpu"):
        self.vocab = list(vocab)
        self.ids, ptr, rat = [], [0], []
        for name in self.vocab:
            entries = list(data.get(name, ()))
            self.ids.append([e["id"] for e in entries])
            rat.extend(_ratios(e["bbox_min"], e["bbox_max"]) for e in entries)
            ptr.append(ptr[-1] + len(entries))
        self.n_classes, self.n_models = len(self.vocab), ptr[-1]
        self.class_ptr_host = np.asarray(ptr, dtype=np.int32)
        self.ratio_host = np.stack(rat).reshape(-1, 2) if rat else np.zeros((0, 2), dtype=np.float64)
        self.to(device)

    def to(self, device):
        self.class_ptr = torch.from_numpy(self.class_ptr_host).to(torch.device(device))
        self.device = self.class_ptr.device                     # (with its index: "cuda" becomes "cuda:0")
        # (one spare row: an empty table still has an address, and the kernel wants it 16-byte aligned)
        self._ratio_buf = torch.zeros(self.n_models + 1, 2, dtype=torch.float64, device=self.device)
        self._ratio_buf[:self.n_models] = torch.from_numpy(self.ratio_host)
        self.ratio = self._ratio_buf[:self.n_models]
        return self

    def count(self, c):
        return int(self.class_ptr_host[c + 1] - self.class_ptr_host[c])

    def id_of(self, c, k):
        return self.ids[int(c)][int(k)]


def _as_layouts(boxes):
    if boxes.dim() not in (2, 3) or boxes.shape[-1] != 6:
        raise ValueError("boxes is [N, 6] or [S, N, 6]")
    return boxes if boxes.dim() == 3 else boxes[None]


def retrieve_models(boxes, objs, room_row, table, dist=False):
    """``boxes`` [N, 6] or [S, N, 6] float32 (row-concatenated rooms, room-normalised, S layouts of the same rows), ``objs`` [N] class
    indices, ``room_row`` [N] every row's room row -> ``choice`` int32 of the boxes' leading shape: the index within the row's class,
    -1 for a room row, a class without models and a class outside the table (and ``dist`` float64, NaN there).  One launch on the
    current stream; nothing is read back."""
    b3 = _as_layouts(boxes)
    if b3.dtype != torch.float32 or not b3.is_cuda:
        raise ValueError("retrieve_models takes float32 boxes on the device (retrieve_models_torch runs anywhere)")
    b3 = b3.contiguous()
    S, N = int(b3.shape[0]), int(b3.shape[1])
    dev = b3.device
    if table.device != dev:
        raise ValueError("the table lives on %s, the boxes on %s" % (table.device, dev))
    objs = objs.to(device=dev, dtype=torch.int32).contiguous()
    room_row = room_row.to(device=dev, dtype=torch.int32).contiguous()
    if objs.numel() != N or room_row.numel() != N:
        raise ValueError("objs and room_row name every row")
    choice = torch.empty(S, N, dtype=torch.int32, device=dev)
    d = torch.empty(S, N, dtype=torch.float64, device=dev) if dist else None
    into(b3, objs, room_row, table, choice, d)
    shape = boxes.shape[:-1]
    return (choice.reshape(shape), d.reshape(shape)) if dist else choice.reshape(shape)


def into(boxes, objs, room_row, table, choice, dist=None):
    """the bare launch over caller-owned buffers (contiguous; boxes [S, N, 6] float32, objs / room_row int32 [N], choice int32 [S, N],
    dist float64 [S, N] or None): allocates nothing - what a stream capture records"""
    S, N = int(boxes.shape[0]), int(boxes.shape[1])
    P = _lib.ptr
    _lib.check(_lib.lib().sln_mesh_retrieve(P(boxes), P(room_row), P(objs), P(table.class_ptr), table.n_classes, P(table._ratio_buf),
                                            table.n_models, S, N, P(choice), P(dist), _lib.current_stream_ptr()), "sln_mesh_retrieve")


def _argmin_np(d):
    """np.argmin along the last axis of d [n, K] (K >= 1) without leaning on a library's tie or NaN rule: the first NaN if there is one,
    else the first position of the minimum"""
    K = d.shape[1]
    ar = torch.arange(K, device=d.device)
    nan = torch.isnan(d)
    first_nan = torch.where(nan, ar, K).min(dim=1).values
    low = torch.where(nan, torch.full_like(d, float("inf")), d).min(dim=1).values
    first_min = torch.where(d == low[:, None], ar, K).min(dim=1).values
    return torch.where(first_nan < K, first_nan, first_min)


def retrieve_models_torch(boxes, objs, room_row, table, dist=False, max_cells=1 << 22):
    """``retrieve_models`` in torch ops, on the boxes' device, with the kernel's order of operations (see the module docstring)."""
    b3 = _as_layouts(boxes).float()
    S, N = int(b3.shape[0]), int(b3.shape[1])
    dev = b3.device
    objs = objs.to(dev).long().reshape(-1)
    room_row = room_row.to(dev).long().reshape(-1)
    ptr = torch.from_numpy(table.class_ptr_host.astype(np.int64)).to(dev)
    ratio = torch.from_numpy(table.ratio_host).to(dev)
    ar = torch.arange(N, device=dev)
    ok = (room_row >= 0) & (room_row < N) & (room_row != ar) & (objs >= 0) & (objs < table.n_classes)
    cls = torch.where(ok, objs, torch.zeros_like(objs))
    count = torch.where(ok, ptr[cls + 1] - ptr[cls], torch.zeros_like(cls)) if table.n_classes else torch.zeros_like(cls)
    ok = ok & (count > 0)
    rm = b3[:, room_row.clamp(0, max(N - 1, 0))]
    ex, ey, ez = rm[..., 3], rm[..., 4], rm[..., 5]
    x0, x1 = b3[..., 0] * ex, b3[..., 3] * ex
    y0, y1 = b3[..., 1] * ey, b3[..., 4] * ey
    z0, z1 = b3[..., 2] * ez, b3[..., 5] * ez
    dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
    r0, r1 = (dy / dx).double().reshape(-1), (dz / dx).double().reshape(-1)            # [S * N]
    choice = torch.full((S * N,), -1, dtype=torch.int32, device=dev)
    best = torch.full((S * N,), float("nan"), dtype=torch.float64, device=dev)
    cls_all, ok_all = cls.repeat(S), ok.repeat(S)
    for c in torch.unique(cls[ok]).tolist():
        a, b = int(table.class_ptr_host[c]), int(table.class_ptr_host[c + 1])
        t = ratio[a:b]
        rows = torch.nonzero(ok_all & (cls_all == c)).reshape(-1)
        step = max(1, max_cells // (b - a))
        for at in range(0, rows.numel(), step):
            rws = rows[at:at + step]
            d = (t[None, :, 0] - r0[rws, None]).abs() + (t[None, :, 1] - r1[rws, None]).abs()
            k = _argmin_np(d)
            choice[rws] = k.to(torch.int32)
            best[rws] = d.gather(1, k[:, None])[:, 0]
    shape = boxes.shape[:-1]
    return (choice.reshape(shape), best.reshape(shape)) if dist else choice.reshape(shape)


def shell_ratios(data):
    """-> (wall_ratio [W, 2], floor_ratio [W]) float64 numpy of a wall table (metadata/wall_data_wfc.json: a list of dicts with
    ``wall_bbox_min / wall_bbox_max / floor_bbox_min / floor_bbox_max``), as :132-133 and :147-148 form them"""
    wall = np.stack([_ratios(e["wall_bbox_min"], e["wall_bbox_max"]) for e in data]).reshape(-1, 2) if len(data) else np.zeros((0, 2))
    floor = np.array([_ratios(e["floor_bbox_min"], e["floor_bbox_max"])[1] for e in data], dtype=np.float64).reshape(-1)
    return wall, floor


def retrieve_shell(boxes, last_row, wall_ratio, floor_ratio):
    """``boxes`` [N, 6] float32 on the device, ``last_row`` [R] the rooms' room rows, ``wall_ratio`` [W, 2] / ``floor_ratio`` [W] float64
    on the device -> int32 [R, 2]: (wall, floor) index per room, -1 for an empty table.  One launch on the current stream."""
    if boxes.dim() != 2 or boxes.shape[1] != 6 or boxes.dtype != torch.float32 or not boxes.is_cuda:
        raise ValueError("retrieve_shell takes float32 boxes [N, 6] on the device (retrieve_shell_torch runs anywhere)")
    dev = boxes.device
    boxes = boxes.contiguous()
    last_row = last_row.to(device=dev, dtype=torch.int32).contiguous()
    wall_ratio = wall_ratio.to(device=dev, dtype=torch.float64).contiguous()
    floor_ratio = floor_ratio.to(device=dev, dtype=torch.float64).contiguous()
    W = int(floor_ratio.numel())
    if wall_ratio.numel() != 2 * W:
        raise ValueError("wall_ratio [W, 2] and floor_ratio [W] describe the same table")
    R = int(last_row.numel())
    out = torch.empty(R, 2, dtype=torch.int32, device=dev)
    P = _lib.ptr
    _lib.check(_lib.lib().sln_shell_retrieve(P(boxes), P(last_row), R, int(boxes.shape[0]), P(wall_ratio) if W else None,
                                             P(floor_ratio) if W else None, W, P(out), _lib.current_stream_ptr()), "sln_shell_retrieve")
    return out


def retrieve_shell_torch(boxes, last_row, wall_ratio, floor_ratio):
    """``retrieve_shell`` in torch ops on the boxes' device: the room row's [3:6] promoted to float64 first (:124,141), then Y / X, Z / X"""
    dev = boxes.device
    last_row = last_row.to(dev).long().reshape(-1)
    wall_ratio, floor_ratio = wall_ratio.to(dev).double().reshape(-1, 2), floor_ratio.to(dev).double().reshape(-1)
    R, N, W = int(last_row.numel()), int(boxes.shape[0]), int(floor_ratio.numel())
    out = torch.full((R, 2), -1, dtype=torch.int32, device=dev)
    ok = (last_row >= 0) & (last_row < N)
    if W == 0 or not bool(ok.any()):
        return out
    rm = boxes.float()[last_row.clamp(0, N - 1)].double()
    q0, q1 = rm[:, 4] / rm[:, 3], rm[:, 5] / rm[:, 3]
    dw = (wall_ratio[None, :, 0] - q0[:, None]).abs() + (wall_ratio[None, :, 1] - q1[:, None]).abs()
    df = (floor_ratio[None, :] - q1[:, None]).abs()
    got = torch.stack([_argmin_np(dw), _argmin_np(df)], 1).to(torch.int32)
    return torch.where(ok[:, None], got, out)


# ---- the reference's call shapes (models/misc.py) over module-level tables, as its globals suncg_data / object_idx_to_name / wall_data_json ----
_TABLES = {"models": None, "data": None, "wall_data": None}


def configure(suncg_data, object_idx_to_name, wall_data=None, device="cpu"):
    """Stands in for models/misc.py:26-31 (the json tables read at import).  ``device``: where the model table lives; the wrappers below
    launch the kernel for boxes on that device when it is a GPU and use the torch restatement for host tensors."""
    _TABLES["data"] = suncg_data
    _TABLES["models"] = ModelTable(suncg_data, object_idx_to_name, device)
    _TABLES["wall_data"] = wall_data


def _stack(bboxes):
    return torch.stack([b.detach().float().reshape(6) for b in bboxes])


def suncg_retrieve(objs, bboxes):
    """:34-64: ``objs`` the class indices, ``bboxes`` a list of [6] tensors (room-normalised, room row last) -> the ids of all rows
    but the last.  The caller's boxes are not touched (the reference scales the host copy it takes)."""
    table = _TABLES["models"]
    if table is None:
        raise RuntimeError("call retrieve.configure(suncg_data, object_idx_to_name) first (stands in for models/misc.py globals)")
    boxes = _stack(bboxes)
    n = boxes.shape[0]
    cls = torch.as_tensor([int(o) for o in objs], dtype=torch.int32)
    room_row = torch.full((n,), n - 1, dtype=torch.int32)
    if boxes.is_cuda:
        choice = retrieve_models(boxes, cls, room_row, table if table.device == boxes.device else table.to(boxes.device))
    else:
        choice = retrieve_models_torch(boxes, cls, room_row, table)
    choice = choice.cpu().tolist()
    ids = []
    for i in range(n - 1):
        if choice[i] < 0:
            raise ValueError("row %d: class %r has no model to retrieve" % (i, int(cls[i])))     # (np.argmin of an empty list raises, :62)
        ids.append(table.id_of(int(cls[i]), choice[i]))
    return ids


def _shell_choice(boxes, data):
    data = _TABLES["wall_data"] if data is None else data
    if data is None:
        raise RuntimeError("no wall table: pass data= or retrieve.configure(..., wall_data=...)")
    if len(data) == 0:
        raise ValueError("the wall table is empty")
    b = _stack(boxes)
    wall, floor = (torch.from_numpy(x) for x in shell_ratios(data))
    last = torch.tensor([b.shape[0] - 1], dtype=torch.int32)
    fn = retrieve_shell if b.is_cuda else retrieve_shell_torch
    return data, fn(b, last, wall, floor)[0].cpu().tolist()


def wall_retrieve(boxes, data=None):
    """:123-137 -> the chosen dict of ``data``"""
    data, (w, _) = _shell_choice(boxes, data)
    return data[w]


def floor_retrieve(boxes, data=None):
    """:139-152 -> the chosen dict of ``data``"""
    data, (_, f) = _shell_choice(boxes, data)
    return data[f]
