"""Scene tensors shared by tools/gen_golden_scene_pictures.py (which runs the reference's save_images / save_label_depth / save_label on
them) and by test_scene_pictures_host.py / test_scene_pictures_gpu.py.  Our own code: ``np.random.RandomState``, exact float32 values.

Every room is piecewise constant over a grid of cells.  A cell is one of
  empty     no class, depth -1 or lower (the background: the room's minimum)
  solid     one plane at 1
  tie       two planes at 1: the first wins the argmax
  soft      two planes at a / 256 and b / 256 with a + b >= 128
  half      two planes summing to exactly 0.5: NOT empty
  below     two planes summing to 0.49609375 (127 / 256): empty
  far       a solid cell whose depth lies more than 10 above the minimum
Depths are multiples of 1 / 64 and, outside ``far`` cells, below 8.5 - so d = depth - min is exact, below 10 and never 10.  Plane values are
multiples of 2^-8: every summation order gives the same float32 sum.  The workgroup footprint of csrc/scene_pictures.hip is 1 024
pixels: S = 64 gives four workgroups a room (16 image rows each)."""
import functools
import hashlib

import numpy as np

FIXTURE_CASES = ("s4_c41", "s12_c70", "s64_b3_c41", "s256_c70")
KINDS = ("empty", "solid", "tie", "soft", "half", "below", "far")
PX_PER_GROUP = 1024


def _cell(rng, kind, C):
    """-> (depth, {channel: value}) of one cell; channels 1..40 semantic, 41.. depth-hot (any 0 / 1 pattern)"""
    planes = {}
    a, b = sorted(rng.choice(40, 2, replace=False) + 1)
    depth = rng.randint(64, 8 * 64 + 32) / 64.0                           # 1 .. 8.48
    if kind == "empty":
        depth = -1.0
    elif kind == "solid":
        planes[a] = 1.0
    elif kind == "tie":
        planes[a] = planes[b] = 1.0
    elif kind == "soft":
        x = rng.randint(64, 200)
        planes[a], planes[b] = x / 256.0, rng.randint(max(128 - x, 1), 256 - x + 1) / 256.0
    elif kind == "half":
        x = rng.randint(1, 128)
        planes[a], planes[b] = x / 256.0, (128 - x) / 256.0
    elif kind == "below":
        x = rng.randint(1, 127)
        planes[a], planes[b] = x / 256.0, (127 - x) / 256.0
    elif kind == "far":
        planes[a] = 1.0
        depth = rng.randint(12 * 64, 20 * 64) / 64.0
    if C > 41:
        planes[41 + rng.randint(0, C - 41)] = 1.0
    return depth, planes


def _room(rng, S, C, grid, kinds=KINDS):
    img = np.zeros((C, S, S), np.float32)
    step = S // grid
    order = (list(kinds) + [kinds[i] for i in rng.randint(0, len(kinds), grid * grid)])[:grid * grid]      # every kind once, then any
    cells = [order[i] for i in rng.permutation(len(order))]
    for k, kind in enumerate(cells):
        r, c = divmod(k, grid)
        depth, planes = _cell(rng, kind, C)
        sl = (slice(r * step, (r + 1) * step if r < grid - 1 else S), slice(c * step, (c + 1) * step if c < grid - 1 else S))
        img[0][sl] = depth
        for ch, v in planes.items():
            img[ch][sl] = v
    return img


def _fill(img, rows, cols, depth, planes):
    img[:, rows, cols] = 0.0
    img[0, rows, cols] = depth
    for ch, v in planes.items():
        img[ch, rows, cols] = v


@functools.lru_cache(maxsize=None)
def case(name):
    """-> float32 [B, C, S, S] (read-only)"""
    seed = dict(s4_c41=1, s12_c70=2, s64_b3_c41=3, s256_c70=4, s64_b3_c70=5)[name]
    rng = np.random.RandomState(20250000 + seed)
    if name == "s4_c41":                       # one vector a row; four cells: the background, a tie, the two sums around 0.5
        img = np.stack([_room(rng, 4, 41, 2, ("empty", "tie", "half", "below"))])
    elif name == "s12_c70":                    # 144 pixels: a partial last wavefront
        img = np.stack([_room(rng, 12, 70, 3)])
    elif name in ("s64_b3_c41", "s64_b3_c70"):
        # four workgroups a room.  The minimum (another one per room) lies in the LAST workgroup's rows and nowhere else; the maximum
        # below 10 (another one per room) in workgroup b, and every other depth stays at least 0.5 below it
        C = 41 if name.endswith("c41") else 70
        rooms = []
        for b in range(3):
            img = _room(rng, 64, C, 8, ("solid", "tie", "soft", "half", "below", "far"))
            near = img[0] < 10
            img[0][near] = np.minimum(img[0][near], 6.5)
            _fill(img, slice(56, 60), slice(8 * b, 8 * b + 8), -1.0 - 0.25 * b, {})
            _fill(img, slice(16 * b + 4, 16 * b + 8), slice(40, 48), 7.0 + 0.125 * b, {1 + 7 * b: 1.0})
            rooms.append(img)
        img = np.stack(rooms)
    elif name == "s256_c70":                   # save_label_depth's canvas
        img = np.stack([_room(rng, 256, 70, 8)])
    else:
        raise KeyError(name)
    img = np.ascontiguousarray(img, np.float32)
    img.setflags(write=False)
    return img


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def in_domain(img):
    """planes in [0, 1], no d == 10, m > 0 in every room"""
    ok = bool((img[:, 1:41] >= 0).all() and (img[:, 1:41] <= 1).all())
    for room in img:
        d = room[0] - room[0].min()
        ok = ok and not bool((d == 10).any()) and float(d[d < 10].max()) > 0
    return ok


def live_case(name="s64_b3_c70"):
    """-> (dirty image, live [B, C] uint8, clean image): planes without a non-zero value are flagged dead (2: some gradient reader, or
    0) and pre-filled with NaN, depth-hot planes that are all ones are flagged 1 and pre-filled with garbage; one semantic plane of room 1
    is made the constant 1 as well"""
    clean = case(name).copy()
    clean[1, 5] = 1.0
    clean[0, 60:] = 1.0
    B, C = clean.shape[:2]
    live = np.full((B, C), 3, np.uint8)
    dirty = clean.copy()
    for b in range(B):
        for c in range(1, C):
            if not clean[b, c].any():
                live[b, c] = 2 if c % 2 else 0
                dirty[b, c] = np.nan
            elif (clean[b, c] == 1).all():
                live[b, c] = 1
                dirty[b, c] = -7.5e8
    return dirty, live, clean


def status_case():
    """-> image [4, 41, 12, 12]: room 1 has one -inf depth (no d < 10: bit 0), room 2 a constant depth plane (m == 0: bit 1), rooms 0 and 3
    are ordinary"""
    img = np.stack([case("s12_c70")[0, :41]] * 4).copy()
    img[3, 0][img[3, 0] == -1.0] = -1.5                                        # another minimum than room 0's (d stays below 9.99)
    img[1, 0, 7, 3] = -np.inf
    img[2, 0] = 3.25
    return img
