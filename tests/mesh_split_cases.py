"""Shared cases of the edge splitter (host/mesh_prep.py, csrc/mesh_split.hip).  Every coordinate is a multiple of 2^-8 of magnitude
below 16: at most 12 significant bits, a pass adds one, so midpoints are exact in float32 through all passes and areas can be compared
exactly."""
import numpy as np

MAX_EDGE = 0.6

# (size, passes, faces, vertices) at max_edge = 0.6: the figures of the rule's CPU prototype
CUBOIDS = {"cube_1": ((1.0, 1.0, 1.0), 2, 96, 50),
           "wall_slab": ((6.0, 2.75, 0.125), 4, 1200, 602),
           "room_box": ((12.0, 3.0, 9.0), 5, 6144, 3074),
           "small_box": ((0.5, 0.25, 0.5), 1, 16, 10)}


def cuboid(sx, sy, sz, lo=(0.0, 0.0, 0.0)):
    """8 vertices (index 4 ix + 2 iy + iz), 12 outward-wound triangles: a closed surface"""
    v = np.array([[x, y, z] for x in (0.0, sx) for y in (0.0, sy) for z in (0.0, sz)], dtype=np.float32) + np.asarray(lo, dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, dtype=np.int32)


def _tri(points, rot=0):
    v = np.array(points, dtype=np.float32)
    return v, np.roll(np.arange(3, dtype=np.int32), -rot)[None].copy()


def _soup(seed, V, F, span):
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, int(span * 256), size=(V, 3)) / 256.0).astype(np.float32)
    f = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int32)
    return v, f


# the plane triangles: A = (0,0,0), B on the x axis, C above; which edges exceed 0.6 is in the name
_T0 = [(0, 0, 0), (0.25, 0, 0), (0, 0.25, 0)]
_T1 = [(0, 0, 0), (1, 0, 0), (0.5, 0.25, 0)]                 # AB = 1, the others 0.559
_T2A = [(0, 0, 0), (0.5, 0, 0), (0.125, 1, 0)]               # AB = 0.5 unmarked; |A M1|^2 = 0.3477 < |B M2|^2 = 0.4414
_T2B = [(0, 0, 0), (0.5, 0, 0), (0.375, 1, 0)]               # the mirror image: |B M2|^2 is the smaller
_T2TIE = [(0, 0, 0), (0.5, 0, 0), (0.25, 1, 0)]              # isosceles: both diagonals 0.5^2 + 0.375^2
_T3 = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]


def cases():
    """name -> (v float32 [V, 3], f int32 [F, 3])"""
    out = {name: cuboid(*size) for name, (size, _, _, _) in CUBOIDS.items()}
    out["tri_0_marked"] = _tri(_T0)
    out["tri_3_marked"] = _tri(_T3)
    for rot in range(3):                                       # the marked / unmarked edge at every position k
        out["tri_1_marked_k%d" % rot] = _tri(_T1, rot)
        out["tri_2_marked_a_k%d" % rot] = _tri(_T2A, rot)
        out["tri_2_marked_b_k%d" % rot] = _tri(_T2B, rot)
        out["tri_2_marked_tie_k%d" % rot] = _tri(_T2TIE, rot)
    # a repeated index (an edge of length 0 and one edge used twice) next to a proper face
    out["repeated_index"] = (np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0.5, 0.5, 1)], dtype=np.float32),
                             np.array([(0, 0, 1), (1, 2, 3)], dtype=np.int32))
    out["zero_area"] = (np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], dtype=np.float32), np.array([(0, 1, 2)], dtype=np.int32))
    # the same triangle twice over duplicate vertices, the second copy starting at another corner
    p = [(0, 0, 0), (1.5, 0, 0.25), (0.25, 1.25, 0.5)]
    out["unwelded_pair"] = (np.array(p + [p[1], p[2], p[0]], dtype=np.float32), np.array([(0, 1, 2), (5, 3, 4)], dtype=np.int32))
    out["soup_40_60"] = _soup(11, 40, 60, 2.0)
    for n in (255, 256, 257):                                  # around the workgroup size of the kernels
        out["soup_%d" % n] = _soup(n, 100, n, 1.5)
    out["no_split"] = cuboid(0.25, 0.25, 0.25, lo=(1.0, 2.0, 3.0))
    return out


def quad_room(X=4.0, Y=2.75, Z=5.0):
    """A room whose shell is ONE quad (two triangles) per wall, floor and ceiling, as ``MeshBank.from_arrays(shell=)`` takes it; the
    table boxes equal the room box, so ``place_shell`` scales by exactly 1."""
    box, _ = cuboid(X, Y, Z)
    wall_f = [np.array([(0, 4, 6), (0, 6, 2)]), np.array([(0, 2, 3), (0, 3, 1)]), np.array([(4, 5, 7), (4, 7, 6)])]      # z = 0, x = 0, x = X
    floor_v = np.array([(0, 0, 0), (X, 0, 0), (X, 0, Z), (0, 0, Z)], dtype=np.float32)
    ceil_v = floor_v + np.array([0, Y, 0], dtype=np.float32)
    quad = np.array([(0, 1, 2), (0, 2, 3)])
    return dict(wall_v=box, wall_f=wall_f, wall_bbox=np.array([(0, 0, 0), (X, Y, Z)], dtype=np.float32), floor_v=floor_v, floor_f=quad,
                floor_bbox=np.array([(0, 0, 0), (X, 0, Z)], dtype=np.float32), ceil_v=ceil_v, ceil_f=quad[:, ::-1].copy())


def quad_room_inputs():
    """class names, boxes [n, 6] (room-normalised, the room row last) and angle bins of a small scene in ``quad_room()``"""
    names = ["bed", "table", "__room__"]
    boxes = np.array([[0.15, 0.0, 0.2, 0.5, 0.25, 0.55], [0.6, 0.0, 0.3, 0.85, 0.3, 0.5], [0, 0, 0, 4.0, 2.75, 5.0]], dtype=np.float32)
    angles = np.array([3.0, 10.0, 0.0], dtype=np.float32)
    meshes = {"bed": cuboid(2.0, 0.5, 1.5), "table": cuboid(1.0, 0.75, 1.0)}
    return names, boxes, angles, meshes
