"""Looking at layouts on the device: the top-down picture of the reference's ``testing/test_plot2d.py::plot2d`` for S layouts x R rooms
in one launch, and footprint heat maps.

  * ``plot_tables``       - the two per-row tables the kernels read: draw rank (``nyu_class_order``, :25-29) and colour (``mapped_colors``,
    :30-71), built once on the host from the class names; the kernels know nothing of vocabularies;
  * ``layout_plot``       - winner-row image and RGB image of every (layout, room) (sln_layout_plot);
  * ``layout_footprints`` - per object row and pixel, the number of layouts whose rotated footprint covers the pixel
    (sln_layout_footprint_counts); ``sampling.layout_counts`` reduces a layout to one pixel per object, its centre;
  * ``plot2d``            - the reference's call shape for one room.

Geometry (include/sln_hip.h has the full statement): a row's ring is ``evaluate.cuboid_iou``'s; the image is ``size`` x ``size`` over
[0, 1]^2 with pixel (r, c) centred at x = (c + 0.5) / size, z = (r + 0.5) / size - row 0 at z ~ 0, what the reference's ``1 - z``
(:124) under matplotlib's y-up axes puts on screen; among the drawn rows that cover a pixel the greatest (rank, row) wins.

The ``*_torch`` functions restate both kernels in torch ops (CPU tensors, the host-side tests), as ``evaluate.*_torch`` do.
"""
import os
import warnings

import torch

from .. import _lib
from . import evaluate as _E

# testing/test_plot2d.py:10-13 (valid_classes): the class list plot2d indexes ``objs`` with
PLOT2D_CLASSES = ("__room__", "curtain", "shower_curtain", "dresser", "counter", "bookshelf", "picture", "mirror",
                  "floor_mat", "chair", "sink", "desk", "table", "lamp", "door", "clothes", "person", "toilet",
                  "cabinet", "floor", "window", "blinds", "wall", "pillow", "whiteboard", "bathtub", "television",
                  "night_stand", "sofa", "refridgerator", "bed", "shelves")
# :16-20
NYU_CLASS_ORIG = ('wall', 'floor', 'cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf',
                  'picture', 'counter', 'blinds', 'desk', 'shelves', 'curtain', 'dresser', 'pillow', 'mirror', 'floor_mat',
                  'clothes', 'ceiling', 'books', 'refridgerator', 'television', 'paper', 'towel', 'shower_curtain',
                  'box', 'whiteboard', 'person', 'night_stand', 'toilet', 'sink', 'lamp', 'bathtub', 'bag',
                  'otherstructure', 'otherfurniture', 'otherprop')
# :25-29: what comes later is painted on top (television above most things, bed last)
NYU_CLASS_ORDER = ('wall', 'floor', 'cabinet', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture',
                   'counter', 'blinds', 'desk', 'shelves', 'curtain', 'dresser', 'pillow', 'mirror', 'floor_mat',
                   'clothes', 'ceiling', 'books', 'refridgerator', 'paper', 'towel', 'shower_curtain',
                   'box', 'whiteboard', 'person', 'night_stand', 'toilet', 'sink', 'lamp', 'bathtub', 'bag',
                   'otherstructure', 'otherfurniture', 'otherprop', 'television', 'bed')
# :30-71, in NYU_CLASS_ORIG order
MAPPED_COLORS = ((174, 199, 232), (152, 223, 138), (31, 119, 180), (255, 187, 120), (188, 189, 34), (140, 86, 75), (255, 152, 150),
                 (214, 39, 40), (197, 176, 213), (148, 103, 189), (196, 156, 148), (23, 190, 207), (178, 76, 76), (247, 182, 210),
                 (66, 188, 102), (219, 219, 141), (140, 57, 197), (202, 185, 52), (51, 176, 203), (200, 54, 131), (92, 193, 61),
                 (78, 71, 183), (172, 114, 82), (255, 127, 14), (91, 163, 138), (153, 98, 156), (140, 153, 101), (158, 218, 229),
                 (100, 125, 154), (178, 127, 135), (120, 185, 128), (146, 111, 194), (44, 160, 44), (112, 128, 144), (96, 207, 209),
                 (227, 119, 194), (213, 92, 176), (94, 106, 211), (82, 84, 163), (100, 85, 144))
DO_NOT_VIS = _E.DO_NOT_VIS                # :74 (with '__room__', which the callers here name themselves)
FLOOR_RGB = MAPPED_COLORS[NYU_CLASS_ORIG.index("floor")]      # :115-117
STAGE_ROWS = 256                          # rows of one room sln_layout_plot stages at once (longer rooms go in chunks)


def pack_rgb(rgb):
    return int(rgb[0]) | int(rgb[1]) << 8 | int(rgb[2]) << 16


def _rgb_i32(rgb):
    """the packed colours as int32 bits (a uint32 tensor is reinterpreted: no cast kernel is needed for it)"""
    return (rgb.view(torch.int32) if rgb.dtype == torch.uint32 else rgb.to(torch.int32)).contiguous()


def plot_tables(objs, vocab_names):
    """objs [O] (class indices into ``vocab_names``) -> (rank [O] int32, rgb [O] uint32), on ``objs``' device.  rank =
    nyu_class_order.index(name) (:118), -1 for '__room__' and the do_not_vis classes (:74,86); rgb =
    mapped_colors[nyu_class_orig.index(name)] (:122) as r | g << 8 | b << 16.  A drawn class outside the nyu list raises ValueError
    (the reference's ``.index`` does)."""
    names = list(vocab_names)
    rank, rgb = [], []
    for i in objs.cpu().to(torch.int64).tolist():
        name = names[i]
        if name == "__room__" or name in DO_NOT_VIS:
            rank.append(-1)
            rgb.append(pack_rgb(FLOOR_RGB))
            continue
        if name not in NYU_CLASS_ORDER or name not in NYU_CLASS_ORIG:
            raise ValueError("%r is not in list (nyu_class_order)" % name)
        rank.append(NYU_CLASS_ORDER.index(name))
        rgb.append(pack_rgb(MAPPED_COLORS[NYU_CLASS_ORIG.index(name)]))
    return (torch.tensor(rank, dtype=torch.int32, device=objs.device), torch.tensor(rgb, dtype=torch.uint32, device=objs.device))


def _check(what, boxes, angles, room_of_row, rank, size, **more):
    _E._check_layouts(boxes)
    S, O, _ = boxes.shape
    tensors = dict(boxes=boxes, angles=angles, room_of_row=room_of_row, rank=rank, **more)
    for name, t in tensors.items():                     # (a host pointer handed to the kernel is a fault, not an exception)
        if t is not None and (not torch.is_tensor(t) or t.device.type != "cuda" or t.device != boxes.device):
            raise _lib.SlnError("%s runs on the MI355X only (no CPU fallback): %s must be a tensor on boxes' cuda device; "
                                "%s_torch restates it for CPU tensors" % (what, name, what))
    if angles.shape != (S, O) or rank.shape != (O,):
        raise ValueError("angles must be [S, O], rank [O]")
    if not 1 <= int(size) <= 1024:
        raise ValueError("size must be in [1, 1024]")
    _E._check_rooms(room_of_row, O)
    return S, O


def layout_plot(boxes, angles, room_of_row, rank, rgb, size=256, room_id=None, n_rooms=None, want_winner=True, want_rgb=True):
    """boxes [S, O, 6], angles [S, O] (float bins; integer tensors are converted), room_of_row / room_id [O] as in
    ``evaluate.cuboid_iou``, rank / rgb [O] from ``plot_tables`` -> (winner [S, R, size, size] int32 or None,
    image [S, R, size, size, 3] uint8 or None)."""
    S, O = _check("layout_plot", boxes, angles, room_of_row, rank, size, rgb=rgb, room_id=room_id)
    if rgb.shape != (O,) or not (want_winner or want_rgb):
        raise ValueError("rgb must be [O]; one of want_winner / want_rgb is needed")
    dev = boxes.device
    if room_id is None:
        room_id, n_rooms = _E._room_ids(room_of_row)
    elif room_id.shape != (O,):
        raise ValueError("room_id must be [O]")
    elif n_rooms is None:
        n_rooms = int(room_id.max()) + 1 if O else 0    # (one read of the table, as _room_ids does)
    R, N = int(n_rooms), int(size)
    b, a = boxes.float().contiguous(), angles.float().contiguous()
    rr, rid = room_of_row.to(torch.int32).contiguous(), room_id.to(torch.int32).contiguous()
    rk, col = rank.to(torch.int32).contiguous(), _rgb_i32(rgb)
    winner = torch.empty(S, R, N, N, dtype=torch.int32, device=dev) if want_winner else None
    image = torch.empty(S, R, N, N, 3, dtype=torch.uint8, device=dev) if want_rgb else None
    for s0 in range(0, S, 65535):                       # (the layout index is a grid axis)
        n = min(65535, S - s0)
        _lib.check(_lib.lib().sln_layout_plot(_lib.ptr(b[s0:]), _lib.ptr(a[s0:]), _lib.ptr(rr), _lib.ptr(rid), _lib.ptr(rk), _lib.ptr(col), R, n, O, N,
                                              _lib.ptr(winner[s0:]) if want_winner else None, _lib.ptr(image[s0:]) if want_rgb else None,
                                              _lib.current_stream_ptr()), "sln_layout_plot")
    return winner, image


def layout_footprints(boxes, angles, room_of_row, rank, size=100, counts=None):
    """boxes [S, O, 6], angles [S, O] -> counts [O, size, size] int32 (+= into ``counts``): the number of layouts whose ring of row o
    covers the pixel, for the rows with rank >= 0 (the other planes are not touched)."""
    S, O = _check("layout_footprints", boxes, angles, room_of_row, rank, size, counts=counts)
    N = int(size)
    counts = torch.zeros(O, N, N, dtype=torch.int32, device=boxes.device) if counts is None else counts
    if counts.shape != (O, N, N) or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous [O, size, size] int32 tensor")
    b, a = boxes.float().contiguous(), angles.float().contiguous()
    rr, rk = room_of_row.to(torch.int32).contiguous(), rank.to(torch.int32).contiguous()
    _lib.check(_lib.lib().sln_layout_footprint_counts(_lib.ptr(b), _lib.ptr(a), _lib.ptr(rr), _lib.ptr(rk), S, O, N, _lib.ptr(counts),
                                                      _lib.current_stream_ptr()), "sln_layout_footprint_counts")
    return counts


def _rows(x, dtype):
    """a tensor, or the reference's list of per-row tensors / numbers (test.py:46-53) -> one tensor"""
    if torch.is_tensor(x):
        return x.detach().to(dtype)
    return torch.stack([torch.as_tensor(v).detach().to(dtype) for v in x])


def save_png(image, save_path):
    """write the [H, W, 3] uint8 picture as a PNG.  A path without an extension gets '.png', as ``plt.savefig(save_path)`` (:140)
    gives it; a file object is written to as it is.  -> the path written (None for a file object or when PIL is missing: a warning)"""
    try:
        from PIL import Image
    except ImportError:
        warnings.warn("plot2d: PIL is not installed, %r was not written" % (save_path,))
        return None
    if isinstance(save_path, (str, os.PathLike)):
        save_path = os.fspath(save_path)
        if not os.path.splitext(save_path)[1]:
            save_path += ".png"
    Image.fromarray(image.cpu().numpy()).save(save_path, format="PNG")
    return save_path if isinstance(save_path, str) else None


def plot2d(boxes, angles, objs, save_path=None, size=256):
    """testing/test_plot2d.py::plot2d for one room: boxes [O, 6] (room row last), angles [O], objs [O] in ``PLOT2D_CLASSES`` indices,
    each a tensor or the reference's list of per-row tensors / numbers (test.py:46-53) -> the [size, size, 3] uint8 picture.  The
    reference's callers hold CPU data (its plot2d calls ``.numpy()``): such input is copied to the current cuda device, drawn there by
    sln_layout_plot and the picture comes back to the CPU; cuda input stays on its device.  Without a device this raises
    (there is no CPU fallback; ``layout_plot_torch`` is the restatement).  ``save_path``: see ``save_png``."""
    boxes, angles = _rows(boxes, torch.float32), _rows(angles, torch.float32).reshape(-1)
    objs = _rows(objs, torch.int64).reshape(-1)
    O = boxes.shape[0]
    if boxes.dim() != 2 or boxes.shape[1] != 6 or angles.shape != (O,) or objs.shape != (O,):
        raise ValueError("plot2d takes boxes [O, 6], angles [O] and objs [O]")
    home = boxes.device
    if home.type != "cuda":
        if not torch.cuda.is_available():
            raise _lib.SlnError("plot2d draws on the MI355X only (no CPU fallback) and no device is visible")
        boxes = boxes.cuda()
    dev = boxes.device
    rank, rgb = plot_tables(objs.cpu(), PLOT2D_CLASSES)
    rr = torch.full((O,), O - 1, dtype=torch.int32, device=dev)
    _, image = layout_plot(boxes[None], angles.to(dev)[None], rr, rank.to(dev), rgb.to(dev), size=size,
                           room_id=torch.zeros(O, dtype=torch.int32, device=dev), n_rooms=1, want_winner=False)
    image = image[0, 0].to(home)
    if save_path is not None:
        save_png(image, save_path)
    return image


# ------------------------------------------------------------------------------------------------------------------------------
# torch restatements
# ------------------------------------------------------------------------------------------------------------------------------
def rings_torch(boxes, angles, room_of_row, dtype=torch.float64):
    """[..., O, 4, 2] rings in (x, z): ``evaluate.cuboids_torch``'s, with the NaN of a non-finite height that the reference's
    3 x 3 rotation (0 * y, :98-110) carries into x and z"""
    ring, h0, h1 = _E.cuboids_torch(boxes, angles, room_of_row, dtype)
    return ring + (0 * h0 + 0 * h1)[..., None, None]


def coverage_torch(ring, size):
    """ring [..., 4, 2] -> [..., size, size] bool: the pixels whose centre the ring covers (the device function ``covers`` of
    csrc/layout_plot.hip, statement for statement, in ``ring``'s dtype)"""
    N = int(size)
    p = ((torch.arange(N, device=ring.device).to(ring.dtype) + 0.5) / N)
    px, pz = p[None, :], p[:, None]
    x, z = ring[..., 0], ring[..., 1]
    e = lambda v: v[..., None, None]
    pos = torch.ones(ring.shape[:-2] + (N, N), dtype=torch.bool, device=ring.device)
    neg = pos.clone()
    for k in range(4):
        ax, az, bx, bz = x[..., k], z[..., k], x[..., (k + 1) % 4], z[..., (k + 1) % 4]
        ek = e(bx - ax) * (pz - e(az)) - e(bz - az) * (px - e(ax))
        pos &= ek >= 0
        neg &= ek <= 0
    # (fminf / fmaxf skip a NaN corner; such a ring has failed above)
    xs, zs = torch.nan_to_num(x, nan=0.0), torch.nan_to_num(z, nan=0.0)
    inbox = (px >= e(xs.amin(-1))) & (px <= e(xs.amax(-1))) & (pz >= e(zs.amin(-1))) & (pz <= e(zs.amax(-1)))
    return (pos | neg) & inbox & e(_E._shoelace(ring) != 0)


def layout_plot_torch(boxes, angles, room_of_row, rank, rgb, size=256, room_id=None, n_rooms=None, dtype=torch.float64):
    """layout_plot as torch ops in ``dtype`` -> (winner [S, R, size, size] int32, image [S, R, size, size, 3] uint8)"""
    S, O, _ = boxes.shape
    dev = boxes.device
    if room_id is None:
        room_id, n_rooms = _E._room_ids(room_of_row)
    R, N = int(n_rooms), int(size)
    ring = rings_torch(boxes, angles, room_of_row, dtype)
    rank_l, rid_l, rr_l = rank.cpu().tolist(), room_id.cpu().tolist(), room_of_row.cpu().tolist()
    best = torch.full((S, R, N, N), -1, dtype=torch.int64, device=dev)                  # (rank, row) as one key; the max does not depend on the order
    for o in range(O):
        if rank_l[o] < 0 or not (o <= rr_l[o] < O) or not (0 <= rid_l[o] < R):
            continue
        key = (min(rank_l[o], 127) << 24) | o
        cov = coverage_torch(ring[:, o], N)
        best[:, rid_l[o]] = torch.where(cov & (best[:, rid_l[o]] < key), torch.full_like(best[:, rid_l[o]], key), best[:, rid_l[o]])
    row = torch.where(best < 0, torch.zeros_like(best), best & 0xffffff)
    winner = torch.where(best < 0, best, row).to(torch.int32)
    col = _rgb_i32(rgb).to(dev).to(torch.int64) & 0xffffffff
    packed = torch.where(best < 0, torch.full_like(best, pack_rgb(FLOOR_RGB)), col[row])
    image = torch.stack([packed & 255, (packed >> 8) & 255, (packed >> 16) & 255], -1).to(torch.uint8)
    return winner, image


def layout_footprints_torch(boxes, angles, room_of_row, rank, size=100, counts=None, dtype=torch.float64):
    """layout_footprints as torch ops in ``dtype`` -> counts [O, size, size] int32 (+= into ``counts``)"""
    S, O, _ = boxes.shape
    N = int(size)
    counts = torch.zeros(O, N, N, dtype=torch.int32, device=boxes.device) if counts is None else counts
    ring = rings_torch(boxes, angles, room_of_row, dtype)
    rank_l, rr_l = rank.cpu().tolist(), room_of_row.cpu().tolist()
    for o in range(O):
        if rank_l[o] >= 0 and o <= rr_l[o] < O:
            counts[o] += coverage_torch(ring[:, o], N).sum(0).to(torch.int32)
    return counts
