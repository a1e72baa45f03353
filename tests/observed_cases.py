"""Hand-made observations for the observed-target builder (host/observe.py, csrc/observed_target.hip): CPU tensors only, shared by
test_observed_target_host.py (torch definition against a Python-loop restatement) and test_observed_target_gpu.py (kernel against the
torch definition).  Sizes 4, 12 and 96; 1, 3 and 17 rooms, every room with content of its own.

A case is a dict: ``name``, ``depth`` [B, S, S] float32, ``labels`` [B, S, S] uint8, ``status`` (the expected status word per room, or
None where the case is random and only the two implementations are compared) and ``ones`` ((room, plane) pairs that must be exactly 1.0).
"""
import numpy as np
import torch

# 32 classes as DR.class_tables lays them out (wall first, three classes without a depth-hot channel, 29 with one) over NYU channels
# picked so that eight channels (5, 9, 13, 17, 25, 29, 33, 37) belong to no class; the depth channels are not in class order
CHAN = [0, 21, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19, 20, 22, 23, 24, 26, 27, 28, 30, 31, 32, 34, 35, 36, 38, 39]
DCH = [-1, -1, -1] + [int(k) for k in np.random.default_rng(5).permutation(29)]
NCH = 70
WALL = CHAN[0] + 1
OWNED = [c + 1 for c in CHAN]                                   # label bytes some class has
UNOWNED = [v for v in range(1, 41) if v not in OWNED]
BAD_BYTE, UNKNOWN, NO_WALL, NO_READING = 1, 2, 4, 8


def plane_of(label):
    """the depth-hot plane of the class with label byte ``label`` (None: wall / floor / ceiling have none)"""
    k = DCH[OWNED.index(label)]
    return None if k < 0 else 41 + k


def _room(rng, S, labels=None, lo=0.5, hi=9.0):
    """a clean random room: every pixel labelled with a class of the tables (or 0) and a reading"""
    pool = np.asarray([0] + OWNED if labels is None else labels, dtype=np.uint8)
    lab = pool[rng.integers(0, len(pool), (S, S))]
    dep = rng.uniform(lo, hi, (S, S)).astype(np.float32)
    return dep, lab


def _case(name, rooms, status=None, ones=()):
    depth = torch.from_numpy(np.stack([r[0] for r in rooms]).astype(np.float32))
    labels = torch.from_numpy(np.stack([r[1] for r in rooms]).astype(np.uint8))
    return dict(name=name, depth=depth, labels=labels, status=status, ones=tuple(ones))


def cases():
    rng = np.random.default_rng(2024)
    out = []
    f32 = np.float32

    # a class present in one pixel only: its mean is that pixel's depth
    d, l = _room(rng, 4, labels=[WALL, 3])
    l[2, 1] = 8; d[2, 1] = f32(3.3)
    out.append(_case("one_pixel_class_s4", [(d, l)], status=[0]))

    # a class of the tables absent from a room: its mean falls back to wall_max and its plane is exactly 1.0
    rooms, ones = [], []
    for b, gone in enumerate((4, 12, 40)):
        d, l = _room(rng, 12, labels=[v for v in [0] + OWNED if v != gone])
        l[0, b] = WALL
        rooms.append((d, l)); ones.append((b, plane_of(gone)))
    out.append(_case("absent_class_s12_b3", rooms, status=[0, 0, 0], ones=ones))

    # no wall pixel (room 1 of three): wall_max = 10
    rooms = [_room(rng, 12), _room(rng, 12, labels=[v for v in OWNED if v != WALL]), _room(rng, 12)]
    rooms[0][1][0, 0] = WALL; rooms[2][1][5, 5] = WALL
    out.append(_case("no_wall_s12_b3", rooms, status=[0, NO_WALL, 0]))

    # no reading anywhere: every label drops out, every mean is wall_max = 10
    d, l = _room(rng, 4, labels=OWNED)
    d[:] = f32(0.0); d[1] = f32(np.nan); d[2] = f32(16.0); d[3] = f32(-2.0)
    out.append(_case("no_reading_s4", [(d, l)], status=[NO_WALL | NO_READING], ones=[(0, p) for p in range(41, 70)]))

    # exactly 15 is a reading, the next float32 is not
    d, l = _room(rng, 4, labels=[WALL, 7])
    d[0, 0] = f32(15.0); l[0, 0] = WALL
    d[0, 1] = np.nextafter(f32(15.0), f32(np.inf)); l[0, 1] = WALL
    d[1, 0] = f32(15.0); l[1, 0] = 7
    d[1, 1] = np.nextafter(f32(15.0), f32(np.inf)); l[1, 1] = 7
    out.append(_case("fifteen_and_next_s4", [(d, l)], status=[NO_READING]))

    # 0, negative, NaN and +-inf depths under a label
    rooms = []
    bad = [f32(0.0), f32(-0.0), f32(-1.0), f32(np.nan), f32(np.inf), f32(-np.inf), f32(-1e-30), f32(1e30)]
    for b in range(3):
        d, l = _room(rng, 12, labels=OWNED)
        for k, v in enumerate(bad):
            d[(k + b) % 12, (3 * k + b) % 12] = v
        rooms.append((d, l))
    out.append(_case("bad_depths_s12_b3", rooms, status=[NO_READING] * 3))

    # label bytes 41 and 255
    d, l = _room(rng, 12)
    l[0, 0] = 41; l[3, 7] = 255; l[11, 11] = 200; l[5, 0] = WALL
    d2, l2 = _room(rng, 12)
    l2[6, 6] = WALL
    out.append(_case("bytes_above_40_s12_b2", [(d, l), (d2, l2)], status=[BAD_BYTE, 0]))

    # labels whose channel no class owns: their semantic planes are still written
    d, l = _room(rng, 12)
    l[0, :8] = np.asarray(UNOWNED, np.uint8); l[1, 0] = WALL
    out.append(_case("unowned_channel_s12", [(d, l)], status=[UNKNOWN]))

    # depths below 2^-9: d * 2^32 is no integer and rint rounds (ties included: odd multiples of 2^-33)
    rooms = []
    for b in range(3):
        d, l = _room(rng, 12, labels=[WALL, 2, 3, 4], lo=2.0 ** -14, hi=2.0 ** -9)
        d[0, :4] = np.asarray([3 * 2.0 ** -33, 5 * 2.0 ** -33, 2.0 ** -33, 2.0 ** -40], f32)
        d[1, :2] = np.asarray([1e-42, 1.17549435e-38], f32)                            # a subnormal and the smallest normal
        rooms.append((d, l))
    out.append(_case("tiny_depths_s12_b3", rooms, status=[0, 0, 0]))

    # the largest sum: 96 x 96 pixels of one class at depth 15
    d = np.full((96, 96), 15.0, f32); l = np.full((96, 96), 4, np.uint8)
    out.append(_case("largest_sum_s96", [(d, l)], status=[NO_WALL]))

    # many rooms, everything mixed
    rooms = []
    for b in range(17):
        d, l = _room(rng, 12)
        hit = rng.random((12, 12))
        d[hit < 0.05] = f32(np.nan); d[(hit >= 0.05) & (hit < 0.1)] = f32(15.5)
        l[hit > 0.97] = np.uint8(41 + b)
        l[(hit > 0.93) & (hit <= 0.97)] = np.uint8(UNOWNED[b % 8])
        rooms.append((d, l))
    out.append(_case("mixed_s12_b17", rooms))
    rooms = []
    for b in range(3):
        d, l = _room(rng, 96, lo=0.01, hi=14.99)
        hit = rng.random((96, 96))
        d[hit < 0.02] = f32(-np.inf); d[(hit >= 0.02) & (hit < 0.04)] = f32(0.0)
        l[hit > 0.99] = np.uint8(250 - b)
        rooms.append((d, l))
    out.append(_case("mixed_s96_b3", rooms))
    return out


def loop_restatement(depth, labels, chan=CHAN, dch=DCH, nch=NCH):
    """The definition once more, pixel by pixel in Python ints and numpy scalars: exact integer sums, float64 means, float32 quotients.
    -> (target [B, nch, S, S] float32 numpy, status [B] int list)"""
    depth, labels = depth.numpy(), labels.numpy()
    B, S, _ = depth.shape
    out = np.zeros((B, nch, S, S), np.float32)
    status = []
    known = set(c + 1 for c in chan)
    for b in range(B):
        lab = np.zeros((S, S), np.int64)
        d0 = np.full((S, S), -1.0, np.float32)
        st = 0
        for y in range(S):
            for x in range(S):
                d, v = depth[b, y, x], int(labels[b, y, x])
                reading = bool(d > 0) and bool(d <= 15)
                if reading:
                    d0[y, x] = d
                if v > 40:
                    st |= BAD_BYTE
                elif v >= 1 and not reading:
                    st |= NO_READING
                elif v >= 1:
                    lab[y, x] = v
                    if v not in known:
                        st |= UNKNOWN
                out[b, 0, y, x] = d0[y, x]
                if lab[y, x] > 0:
                    out[b, lab[y, x], y, x] = 1.0
        cnt, tot, top = {}, {}, {}
        for y in range(S):
            for x in range(S):
                v = int(lab[y, x])
                if v:
                    q = float(d0[y, x]) * 4294967296.0                                  # exact in float64
                    cnt[v] = cnt.get(v, 0) + 1
                    tot[v] = tot.get(v, 0) + int(round(q))                              # Python's round: half to even, as rint
                    top[v] = max(top.get(v, -np.inf), float(d0[y, x]))
        wl = chan[0] + 1
        if wl not in cnt:
            st |= NO_WALL
        wall_max = np.float32(top[wl]) if wl in cnt else np.float32(10.0)
        for c, k in enumerate(dch):
            if k < 0:
                continue
            v = chan[c] + 1
            fill = np.float32((float(tot[v]) * 2.0 ** -32) / float(cnt[v])) if v in cnt else wall_max
            fq = np.float32(fill) / wall_max
            for y in range(S):
                for x in range(S):
                    out[b, 41 + k, y, x] = (d0[y, x] / wall_max) if lab[y, x] == v else fq
        status.append(st)
    return out, status
