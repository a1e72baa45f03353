"""Small layouts for the interpenetration penalty (sln_layout_overlap_penalty, evaluate.overlap_penalty*): boxes [S, O, 6] in room units
(the room row last in its room, its [3:6] the extent), angles [S, O] in float bins of 15 degrees, room_of_row [O], collide [O].
Furniture is written in metres and divided by the extent.  Edge crossings stay well away from grazing in the cases whose gradients
are compared (a-f, h): the angle bins differ by fractions that keep crossing edges far from parallel, no sliver overlaps."""
import torch

EXT = (6.0, 3.0, 5.0)

# (x0, y0, z0, x1, y1, z1) in metres, angle bin
FURNITURE = [((1.0, 0.0, 1.0, 3.0, 1.0, 2.5), 1.3),
             ((2.2, 0.1, 1.6, 4.0, 0.8, 3.4), 4.1),
             ((1.6, 0.3, 2.0, 3.2, 1.5, 3.6), 8.3),
             ((2.6, 0.2, 0.8, 4.6, 1.2, 2.2), 10.4)]


def _room(furniture, ext=EXT):
    """rows of one room: the furniture in room units, then the room row (0, 0, 0, extent) at angle 0"""
    rows = [[v / ext[k % 3] for k, v in enumerate(box)] for box, _ in furniture] + [[0.0, 0.0, 0.0] + list(ext)]
    return rows, [a for _, a in furniture] + [0.0]


def _case(rooms, collide=None, S=1, jitter=0.0, seed=0):
    boxes, angles, rr = [], [], []
    for rows, ang in rooms:
        boxes += rows
        angles += ang
        rr += [len(boxes) - 1] * len(rows)
    b = torch.tensor(boxes, dtype=torch.float64)[None].repeat(S, 1, 1)
    a = torch.tensor(angles, dtype=torch.float64)[None].repeat(S, 1)
    rr = torch.tensor(rr, dtype=torch.int32)
    room_row = rr == torch.arange(len(boxes))
    if jitter:                                                # layouts 1.. differ from layout 0: furniture moved, room rows kept
        g = torch.Generator().manual_seed(seed)
        move = jitter * (torch.rand(S, len(boxes), 1, generator=g, dtype=torch.float64) - 0.5).repeat(1, 1, 6)
        turn = 4 * jitter * (torch.rand(S, len(boxes), generator=g, dtype=torch.float64) - 0.5)
        move[0], turn[0] = 0, 0
        b = torch.where(room_row[None, :, None], b, b + move)
        a = torch.where(room_row[None], a, a + turn)
    if collide is None:
        collide = ~room_row
    return dict(boxes=b.float().contiguous(), angles=a.float().contiguous(), room_of_row=rr, collide=torch.as_tensor(collide).to(torch.uint8))


def _many_rows():
    """(e): one room of 130 rows; rows 3, 20, 64, 65, 100 and 128 collide - the four of (a) and two more that cut into them; the other
    123 pieces of furniture lie all over the room (many on top of each other) and take no part"""
    g = torch.Generator().manual_seed(5)
    lo = torch.rand(129, 3, generator=g, dtype=torch.float64) * torch.tensor([4.5, 1.5, 3.5], dtype=torch.float64)
    size = 0.3 + torch.rand(129, 3, generator=g, dtype=torch.float64) * 1.2
    ang = (torch.rand(129, generator=g, dtype=torch.float64) * 24).tolist()
    rows = [(tuple(lo[k].tolist()) + tuple((lo[k] + size[k]).tolist()), ang[k]) for k in range(129)]
    chosen = [3, 20, 64, 65, 100, 128]
    extra = [((0.6, 0.05, 1.4, 2.0, 0.9, 3.0), 5.6), ((3.0, 0.15, 1.2, 5.0, 1.1, 3.0), 2.2)]
    for k, f in zip(chosen, FURNITURE + extra):
        rows[k] = f
    collide = torch.zeros(130, dtype=torch.bool)
    collide[chosen] = True
    return _case([_room(rows)], collide=collide)


def _swapped():
    rows, ang = _room(FURNITURE)
    rows[1][0], rows[1][3] = rows[1][3], rows[1][0]           # x1 < x0: the ring of row 1 runs clockwise
    return _case([(rows, ang)])


EXT_H = (6.0, 2.0, 5.0)                                       # (heights times a power of two: the ties below are exact in float32)
TIED = [((1.0, 0.0, 1.0, 3.0, 1.0, 2.5), 1.3),                # all stand on the floor (h0 = 0); rows 0 and 1 also end at the same height
        ((2.2, 0.0, 1.6, 4.0, 1.0, 3.4), 4.1),
        ((1.6, 0.0, 2.0, 3.2, 1.5, 3.6), 8.3),
        ((1.8, 1.5, 2.2, 3.0, 1.75, 3.2), 9.0)]               # stands on row 2: their height overlap is exactly 0; above rows 0 and 1

CASES = {
    "a_generic": _case([_room(FURNITURE)]),
    "b_axis_aligned": _case([_room([(b, a) for (b, _), a in zip(FURNITURE, (0.0, 6.0, 12.0, 0.0))])]),
    "c_two_rooms": _case([_room(FURNITURE[:3]), _room(FURNITURE)]),
    "d_three_layouts": _case([_room(FURNITURE)], S=3, jitter=0.05, seed=3),
    "e_many_rows": _many_rows(),
    "f_clockwise": _swapped(),
    "g_disjoint": _case([_room([((0.5, 0.0, 0.5, 1.5, 1.0, 1.5), 1.3), ((2.5, 0.0, 0.5, 3.5, 1.0, 1.5), 4.1), ((0.5, 0.0, 3.0, 1.5, 1.0, 4.0), 8.3),
                                ((2.5, 1.2, 3.0, 3.5, 2.0, 4.0), 8.3), ((2.5, 0.0, 3.0, 3.5, 1.0, 4.0), 10.4)])]),
    "h_height_ties": _case([_room(TIED, EXT_H)]),
    "i_identical": _case([_room([FURNITURE[0], FURNITURE[0], FURNITURE[2]])]),
    "i_zero_width": _case([_room([FURNITURE[0], ((2.5, 0.0, 1.2, 2.5, 1.0, 2.4), 3.0), FURNITURE[2]])]),
}
COMPARED = ["a_generic", "b_axis_aligned", "c_two_rooms", "d_three_layouts", "e_many_rows", "f_clockwise", "h_height_ties"]   # gradients compared
FD_CASES = COMPARED[:6]                                       # a-f: against central differences (h's ties are kinks of the height factor)
FINITE_ONLY = ["i_identical", "i_zero_width"]
