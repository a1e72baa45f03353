"""Cases shared by test_plot2d_host.py and test_plot2d_gpu.py: the exact known-answer rooms, the seeded random layouts with their fp64
reference (computed once per process), and the band of pixels that lie within DELTA of a drawn edge line."""
import functools

import numpy as np
import torch

from conftest import pkg

# Corner coordinates are O(1) float32 after about ten rounded operations and one sinf / cosf: within ~1e-6 of the fp64 ring.  A pixel
# whose centre is at least ten times that from every drawn edge line is decided alike in both precisions.
DELTA = 1e-5
SIZES = (8, 17, 100, 128)


def P():
    return pkg("host.plot2d")


def cls(name):
    return P().PLOT2D_CLASSES.index(name)


# the reference's own example call (test.py:46-53, "Please follow this data format when calling the plot2d function"): a list of [6]
# CPU tensors, a list of 0-d tensors, a list of ints
def reference_example():
    boxes = [[0.31150928139686584, 0.3127100169658661, 0.003096628002822399, 0.7295752763748169, 0.8262581825256348, 0.054250866174697876],
             [-0.06599953025579453, 0.017223943024873734, 0.2885378897190094, 0.2573782205581665, 0.7553179860115051, 0.42857787013053894],
             [0.5567594766616821, 0.017786923795938492, 0.142490953207016, 0.9046159982681274, 0.31667089462280273, 0.6691973209381104],
             [0.6205720901489258, 0.018211644142866135, 0.8416993021965027, 0.8348240852355957, 0.3893248736858368, 0.963701605796814],
             [0.171146959066391, 0.017671708017587662, 0.8085968494415283, 0.4601595997810364, 0.5026606321334839, 0.9657217264175415],
             [0.0, 0.0, 0.0, 1.0, 0.7327236533164978, 0.9278678297996521]]
    rots = [0.0008550407364964485, 18.074506759643555, 6.062503337860107, 12.16077995300293, 12.012971878051758, 0.0]
    return ([torch.from_numpy(np.array(x)).float() for x in boxes], [torch.from_numpy(np.array(x)).float() for x in rots], [20, 18, 30, 3, 11, 0])


# ------------------------------------------------------------------------------------------------------------------------------
# exact known answers: N = 8 (centres at odd / 16), dyadic coordinates, room extent 1
# ------------------------------------------------------------------------------------------------------------------------------
ROOM = [0, 0, 0, 1, 1, 1]
KNOWN_N = 8


def known_cases():
    """name -> (class names, boxes [O, 6], angle bins [O]); the room row is last.  Bin 12 (a half turn: the same footprint, up to the
    1e-7 of sinf(float32(pi))) is used only where no edge passes through a line of centres."""
    b = lambda x0, z0, x1, z1: [x0, 0, z0, x1, 0.5, z1]
    on = b(3 / 16, 0.25, 11 / 16, 0.75)                                   # x edges exactly on the centres of columns 1 and 5
    return {
        "edge_on_centres": (["bed", "__room__"], [on, ROOM], [0, 0]),
        "swapped_x": (["bed", "__room__"], [b(11 / 16, 0.25, 3 / 16, 0.75), ROOM], [0, 0]),
        "zero_width": (["bed", "__room__"], [b(3 / 16, 0.25, 3 / 16, 0.75), ROOM], [0, 0]),
        "nan": (["bed", "chair", "__room__"], [b(float("nan"), 0.25, 0.5, 0.75), b(0.5, 0.5, 1.0, 1.0), ROOM], [0, 12, 0]),
        "same_class": (["chair", "chair", "__room__"], [b(0.125, 0.125, 0.625, 0.625), b(0.375, 0.375, 0.875, 0.875), ROOM], [12, 0, 0]),
        "order_a": (["bed", "television", "chair", "__room__"],
                    [b(0.25, 0.25, 0.75, 0.75), b(0.5, 0.0, 1.0, 0.5), b(0.0, 0.0, 1.0, 0.375), ROOM], [0, 12, 0, 0]),
        "order_b": (["chair", "television", "bed", "__room__"],
                    [b(0.0, 0.0, 1.0, 0.375), b(0.5, 0.0, 1.0, 0.5), b(0.25, 0.25, 0.75, 0.75), ROOM], [12, 0, 12, 0]),
        "nothing_drawn": (["door", "window", "__room__"], [b(0.25, 0.25, 0.75, 0.75), b(0.0, 0.0, 0.5, 0.5), ROOM], [0, 0, 0]),
    }


def known_inputs(name):
    """-> (boxes [1, O, 6] float32, angles [1, O], room_of_row, rank, rgb, expected winner [N, N] int32), CPU tensors"""
    names, boxes, bins = known_cases()[name]
    objs = torch.tensor([cls(n) for n in names])
    rank, rgb = P().plot_tables(objs, P().PLOT2D_CLASSES)
    O = len(names)
    # the expectation, written out: an axis-aligned rectangle with inclusive edges, empty when it has no width or a NaN coordinate;
    # rows painted in (rank, row) order
    c = (np.arange(KNOWN_N) + 0.5) / KNOWN_N
    want = np.full((KNOWN_N, KNOWN_N), -1, np.int32)
    for _, o in sorted((int(rank[o]), o) for o in range(O) if int(rank[o]) >= 0):
        x0, _, z0, x1, _, z1 = boxes[o]
        if x0 == x1 or z0 == z1:
            continue
        inx = (c >= min(x0, x1)) & (c <= max(x0, x1))
        inz = (c >= min(z0, z1)) & (c <= max(z0, z1))
        want[np.ix_(inz, inx)] = o
    return (torch.tensor(boxes, dtype=torch.float32)[None], torch.tensor(bins, dtype=torch.float32)[None],
            torch.full((O,), O - 1, dtype=torch.int32), rank, rgb, torch.from_numpy(want))


def palette_image(winner, rgb):
    """winner [...] int32, rgb [O] packed -> [..., 3] uint8 (the floor where the winner is -1)"""
    pal = torch.cat([rgb.to(torch.int64) & 0xffffffff, torch.tensor([P().pack_rgb(P().FLOOR_RGB)])])
    p = pal[winner.to(torch.int64)]                                      # (-1 indexes the appended floor entry)
    return torch.stack([p & 255, (p >> 8) & 255, (p >> 16) & 255], -1).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------------------
# seeded random layouts
# ------------------------------------------------------------------------------------------------------------------------------
_DRAWN = ["bed", "television", "chair", "sofa", "table", "desk", "cabinet", "lamp", "night_stand", "shelves", "toilet", "dresser"]
_HIDDEN = ["door", "window", "curtain"]


def _room(rng, S, n_obj, small, hidden=0.15):
    """n_obj object rows + the room row: (class indices [n_obj + 1], boxes [S, n_obj + 1, 6], bins [S, n_obj + 1])"""
    names = []
    for _ in range(n_obj):
        pool = _HIDDEN if rng.random() < hidden else _DRAWN
        names.append(pool[int(rng.integers(0, len(pool)))])
    ext = rng.uniform([0.8, 0.5, 0.8], [1.0, 0.7, 1.0], size=(S, 3))
    size = rng.uniform(0.03, 0.12, size=(S, n_obj, 3)) if small else rng.uniform(0.1, 0.45, size=(S, n_obj, 3))
    lo = rng.uniform(0.02, 0.98 - size)
    b = np.concatenate([lo, lo + size], -1)
    flip = rng.random((S, n_obj)) < 0.15                                    # a decoder may predict x1 < x0
    b[flip] = b[flip][:, [3, 1, 2, 0, 4, 5]]
    b = b / np.concatenate([ext, ext], -1)[:, None]
    room = np.concatenate([np.zeros((S, 1, 3)), ext[:, None]], -1)
    bins = np.concatenate([rng.integers(0, 24, size=(S, n_obj)), np.zeros((S, 1))], 1)
    return [cls(n) for n in names] + [0], np.concatenate([b, room], 1), bins


@functools.lru_cache(maxsize=None)
def random_case(kind, S):
    """kind 'two_rooms' (4 and 11 rows in one call), 'long_room' (one room of stage cap + 1 object rows), 'footprints' (O = 6) or 'one_object'
    -> dict of CPU tensors: boxes [S, O, 6] float32, angles [S, O] float32, objs, room_of_row, room_id, n_rooms, rank, rgb"""
    seed = dict(two_rooms=11, long_room=12, footprints=13, one_object=14)[kind]
    rng = np.random.default_rng([seed, S])
    if kind == "two_rooms":
        parts = [_room(rng, S, 3, False), _room(rng, S, 10, False)]
    elif kind == "long_room":
        # (every drawn edge LINE crosses the whole image and passes within DELTA of about 2e-5 N^2 centres: half of the rows are of classes
        # that are not drawn, which keeps the excluded share near 1 % at N = 128; the stages are walked all the same)
        # stage cap + 1 object rows and the room row: the second stage holds a drawn row (a bed: on top wherever it lies)
        parts = [_room(rng, S, P().STAGE_ROWS + 1, True, hidden=0.5)]
        parts[0][0][P().STAGE_ROWS - 1] = cls("chair")
        parts[0][0][P().STAGE_ROWS] = cls("bed")
    elif kind == "footprints":
        parts = [_room(rng, S, 5, False)]
    else:
        parts = [_room(rng, S, 1, False)]
        parts[0][0][0] = cls("bed")
    objs = torch.tensor(sum((p[0] for p in parts), []))
    boxes = torch.from_numpy(np.concatenate([p[1] for p in parts], 1).astype(np.float32))
    angles = torch.from_numpy(np.concatenate([p[2] for p in parts], 1).astype(np.float32))
    ends = np.cumsum([len(p[0]) for p in parts])
    rr = torch.tensor(sum(([int(e) - 1] * len(p[0]) for p, e in zip(parts, ends)), []), dtype=torch.int32)
    rid = torch.tensor(sum(([i] * len(p[0]) for i, p in enumerate(parts)), []), dtype=torch.int32)
    rank, rgb = P().plot_tables(objs, P().PLOT2D_CLASSES)
    return dict(boxes=boxes, angles=angles, objs=objs, room_of_row=rr, room_id=rid, n_rooms=len(parts), rank=rank, rgb=rgb)


def near_edges(case, N):
    """[S, O, N, N] bool: the pixel centre is closer than DELTA to one of the four edge LINES of the row's ring (fp64); all False for
    rows that are not drawn"""
    ring = P().rings_torch(case["boxes"], case["angles"], case["room_of_row"], torch.float64)
    S, O = ring.shape[:2]
    p = (torch.arange(N, dtype=torch.float64) + 0.5) / N
    px, pz = p[None, :], p[:, None]
    near = torch.zeros(S, O, N, N, dtype=torch.bool)
    for o in range(O):
        if int(case["rank"][o]) < 0:
            continue
        for k in range(4):
            a, b = ring[:, o, k], ring[:, o, (k + 1) % 4]
            d = b - a
            ln = d.norm(dim=-1)
            e = d[:, 0, None, None] * (pz - a[:, 1, None, None]) - d[:, 1, None, None] * (px - a[:, 0, None, None])
            near[:, o] |= (e.abs() < DELTA * ln[:, None, None]) & (ln > 0)[:, None, None]
    return near


@functools.lru_cache(maxsize=None)
def plot_reference(kind, S, N):
    """-> (winner [S, R, N, N], image, excluded [S, R, N, N] bool) of the fp64 restatement"""
    c = random_case(kind, S)
    w, im = P().layout_plot_torch(c["boxes"], c["angles"], c["room_of_row"], c["rank"], c["rgb"], size=N, room_id=c["room_id"], n_rooms=c["n_rooms"])
    near = near_edges(c, N)
    excl = torch.stack([near[:, c["room_id"] == r].any(1) for r in range(c["n_rooms"])], 1)
    return w, im, excl


@functools.lru_cache(maxsize=None)
def footprint_reference(kind, S, N):
    """-> (counts [O, N, N] int32 of the fp64 restatement, slack [O, N, N]: the layouts with an edge within DELTA of the pixel)"""
    c = random_case(kind, S)
    counts = P().layout_footprints_torch(c["boxes"], c["angles"], c["room_of_row"], c["rank"], size=N)
    return counts, near_edges(c, N).sum(0).to(torch.int32)
