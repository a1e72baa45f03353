"""Cases of the rasterizer's backward kernels at face level (test_raster_bwd_ref_host.py proves on the CPU what each one
reaches; the comparison of the kernels with the double-sum reference of oracle/raster_ref.cpp is built on them:
LAB_NOTES section 23).

Geometry is hand-made, `[F, 3, 3]` faces of (x_ndc, y_ndc, z), not rooms:
  (a) two triangles of a quad that overhangs the view (corners at +-1.3 plus a small offset): clipped long edges, outward rows
      as long as the image;
  (b) small random triangles in front of it, each followed by its mirrored copy (what fill_back makes): rows under 64 pixels,
      back-facing faces, occluded inward scans, ownerless faces;
  (c) one zero-area face (three distinct collinear points, exact in fp32);
  (d) a right triangle whose vertices sit exactly on pixel centres, plus its mirror: axis-aligned legs through pixel centres
      (slot unused, slope 0/0);
  (e) a triangle with one vertex one ulp off a pixel centre (ratios around 1e7);
  (f) a triangle that straddles the image border and one wholly outside it;
  padding faces lie wholly outside the view (x in [3, 4]).
An image of a batch takes the "main" set (a)-(d) when its index is even and the "edge" set (a), (c)-(f) with fewer small
triangles when it is odd; both have 25 faces.  Images and incoming gradients are multiples of 1/8 in [-2, 2]: every diff is then
exact in fp32 in any summation order, so kernel and reference take the same `diff > 0` decisions and no element is left out.

Incoming gradients are non-zero on a fraction min(1, (24 / is)^2) of the pixels, and every case carries a seed.  Both serve the host
test's demand on the REFERENCE: the oracle's serial fp32 sum has to lie within half the kernels' allowance of the double sum.  A sum
of n same-signed terms (the outward rows of a small triangle) misses 0.25 sqrt(n) half-ulps of S in about one element of a hundred
whatever the data; thinner gradients keep n of such elements in the low hundreds, and the seed of a case is the first one at
which every element of that case passes (found with the host test's own check; the kernels' output never entered).
"""
from collections import namedtuple

import numpy as np

F_STD = 25
EPS = 1e-3


def _p_of(x, is_):
    """pixel coordinate the rasterizer computes for the NDC coordinate x (fp32 steps of 0.5 * (x * is + is - 1))"""
    f = np.float32
    return f(0.5 * np.float64(f(f(f(x) * f(is_)) + f(is_)) - f(1)))


def _centre(k, is_):
    return np.float32((2.0 * k + 1 - is_) / is_)


def _front(tri):
    """the winding the rasterizer draws (its back-face test, restated)"""
    t = np.asarray(tri, np.float32)
    back = (t[2, 1] - t[0, 1]) * (t[1, 0] - t[0, 0]) < (t[1, 1] - t[0, 1]) * (t[2, 0] - t[0, 0])
    return t[[2, 1, 0]] if back else t


def quad_overhang(seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.05, 0.05, size=(4, 2))
    c = np.array([[-1.3, -1.3], [1.3, -1.3], [1.3, 1.3], [-1.3, 1.3]]) + o
    z = np.array([3.0, 3.5, 4.0, 3.25])                   # a tilted plane: the depth gradient's x, y terms do not cancel
    v = np.concatenate([c, z[:, None]], 1)
    return [_front(v[[0, 1, 2]]), _front(v[[0, 2, 3]])]


def small_triangles(seed, pairs):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(pairs):
        c = rng.uniform(-0.85, 0.85, size=(1, 2))
        xy = c + rng.uniform(-0.3, 0.3, size=(3, 2))
        z = rng.uniform(1.0, 2.5, size=(3, 1))
        t = _front(np.concatenate([xy, z], 1))
        out += [t, t[[2, 1, 0]]]
    return out


def zero_area():
    return [np.array([[-0.25, -0.125, 2.0], [0.25, 0.125, 2.0], [0.75, 0.375, 2.0]], np.float32)]


def pixel_centre_triangle(is_):
    """vertices (k0, k0), (k1, k0), (k0, k1) in pixels, each coordinate exactly an integer after the rasterizer's own arithmetic"""
    ks = [k for k in range(is_) if _p_of(_centre(k, is_), is_) == k]
    lo = [k for k in ks if k >= is_ // 5]
    hi = [k for k in ks if k <= (4 * is_) // 5]
    k0, k1 = lo[0], hi[-1]
    assert k1 > k0
    a, b = _centre(k0, is_), _centre(k1, is_)
    t = _front(np.array([[a, a, 0.9], [b, a, 0.8], [a, b, 0.7]], np.float32))
    return [t, t[[2, 1, 0]]]


def ulp_off_triangle(is_):
    """one vertex the smallest fp32 step of x (and of y) off a pixel centre that still moves its pixel coordinate"""
    k = max(1, is_ // 6)
    out = []
    for c in (k, k + 1):
        x = _centre(c, is_)
        for _ in range(64):
            x = np.nextafter(x, np.float32(2), dtype=np.float32)
            if _p_of(x, is_) != c:
                break
        out.append(x)
    far = _centre(is_ - 1 - k, is_)
    return [_front(np.array([[out[0], out[1], 0.6], [far, _centre(k + 2, is_), 0.65], [_centre(is_ // 2, is_), far, 0.7]], np.float32))]


def border_and_outside():
    return [_front(np.array([[0.7, -0.4, 0.5], [1.6, -0.1, 0.5], [0.9, 0.5, 0.55]], np.float32)),
            _front(np.array([[1.5, 1.5, 0.5], [2.5, 1.6, 0.5], [2.0, 2.4, 0.5]], np.float32))]


def padding(n):
    return [np.array([[3.0, 0.0, 1.0], [4.0, 0.0, 1.0], [3.5, 0.5 + 0.01 * i, 1.0]], np.float32) for i in range(n)]


def geometry(is_, b, F=F_STD):
    """[F, 3, 3] float32 faces of image b of a batch at image size is_"""
    if b % 2 == 0:
        faces = quad_overhang(b) + small_triangles(100 + b, 10) + zero_area() + pixel_centre_triangle(is_)
    else:
        faces = (quad_overhang(b) + small_triangles(100 + b, 6) + zero_area() + pixel_centre_triangle(is_) + ulp_off_triangle(is_) +
                 border_and_outside())
    faces = faces + padding(F - len(faces))
    assert len(faces) == F
    return np.stack([np.asarray(f, np.float32) for f in faces])


def batch_geometry(is_, B, F=F_STD, first=0):
    return np.stack([geometry(is_, first + b, F) for b in range(B)])


def eighths(rng, shape):
    return (rng.integers(-16, 17, size=shape) / 8.0).astype(np.float32)


def sparse_eighths(rng, shape, is_, pixel_axes):
    """multiples of 1/8, non-zero on min(1, (24 / is)^2) of the pixels (all channels of a pixel together)"""
    keep_shape = [n if a in pixel_axes else 1 for a, n in enumerate(shape)]
    keep = rng.uniform(size=keep_shape) < min(1.0, (24.0 / is_) ** 2)
    return eighths(rng, shape) * keep.astype(np.float32)


# seed of every case that does not use 0 (see the module docstring)
SEEDS = {"dense-B8-is64": 1, "dense-B8-is65": 5, "dense-B9-is65": 1, "multi-P1-is64-B1": 1, "multi-P1-is65-B9": 3}


def _rng(name):
    return np.random.default_rng([sum(map(ord, name)), SEEDS.get(name, 0)])


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel-map dense (sln_raster_backward_rgb)
# ---------------------------------------------------------------------------------------------------------------------------------
# first: geometry index of image 0 (0: main set, 1: edge set); index_map: "forward" (nmr_forward's) or "random" (uniform in [-1, F))
Dense = namedtuple("Dense", "name is_ B F C first index_map")
DENSE = (
    [Dense("is%d-g%d" % (s, g), s, 1, F_STD, 3, g, "forward") for s in (8, 64, 65, 128, 130, 257) for g in (0, 1)] +
    [Dense("C%d" % c, 65, 2, F_STD, c, 0, "forward") for c in (1, 4)] +
    [Dense("B2-is64", 64, 2, F_STD, 3, 0, "forward"), Dense("B2-is130", 130, 2, F_STD, 3, 0, "forward"),
     Dense("B8-is64", 64, 8, F_STD, 3, 0, "forward"), Dense("B8-is65", 65, 8, F_STD, 3, 0, "forward"),
     Dense("B9-is65", 65, 9, F_STD, 3, 0, "forward"), Dense("B9-is130", 130, 9, F_STD, 3, 0, "forward"),
     Dense("B17-is130", 130, 17, F_STD, 3, 0, "forward"),
     Dense("nosplit-F5504", 64, 2, 5504, 3, 0, "forward")] +
    [Dense("random-map-is%d" % s, s, 2, F_STD, 3, 0, "random") for s in (64, 65, 130)]
)


def dense_inputs(c):
    """faces [B,F,3,3], fi [B,is,is] int32, rgb / grad [B,is,is,C] (multiples of 1/8)"""
    from oracle import raster_ref as rr
    rng = _rng("dense-" + c.name)
    faces = batch_geometry(c.is_, c.B, c.F, c.first)
    if c.index_map == "forward":
        fi = rr.nmr_forward(faces, c.is_, 0.001, 100.0)[0]
    else:
        fi = rng.integers(-1, c.F, size=(c.B, c.is_, c.is_)).astype(np.int32)
    rgb = eighths(rng, (c.B, c.is_, c.is_, c.C))
    grad = sparse_eighths(rng, (c.B, c.is_, c.is_, c.C), c.is_, (0, 1, 2))
    return faces, fi, rgb, grad


def room_inputs(is_=128):
    """the room of test_raster_gpu.py::test_texture_sampling_and_backwards with images in multiples of 1/8"""
    import torch
    from oracle import raster_ref as rr
    V, F, ranges, box = rr.synth_room(3, n_objects=4, target_faces=600)
    K, R, t = rr.get_cam_mat(torch.from_numpy(box))
    f = torch.from_numpy(F)[None]
    f2 = torch.cat((f, f[:, :, [2, 1, 0]]), 1)
    faces = rr.vertices_to_faces(rr.project(torch.from_numpy(V)[None], K, R, t, 512), f2).contiguous().numpy()
    fi = rr.nmr_forward(faces, is_, 0.001, 100.0)[0]
    rng = _rng("dense-room")
    return faces, fi, eighths(rng, (1, is_, is_, 3)), sparse_eighths(rng, (1, is_, is_, 3), is_, (0, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel-map multi (sln_raster_backward_rgb_multi)
# ---------------------------------------------------------------------------------------------------------------------------------
Multi = namedtuple("Multi", "name is_ B P")
MULTI = [Multi("P%d-is%d-B%d" % (p, s, b), s, b, p) for p in (1, 3, 64) for s in (64, 65, 130) for b in (1, 9)]


def multi_inputs(c):
    """faces, fi, passes [P][B,3,is,is], grads [P][B,3,is,is]: images as the Renderer returns them (channels first, rows flipped).
    P = 64: 0/1 class masks - pass p is 1 where a blocky class map equals p; pass 63 is the only non-zero pass on the top band of
    the image, the passes 5, 17 and 40-50 are zero everywhere."""
    from oracle import raster_ref as rr
    rng = _rng("multi-" + c.name)
    faces = batch_geometry(c.is_, c.B)
    fi = rr.nmr_forward(faces, c.is_, 0.001, 100.0)[0]
    shape = (c.B, 3, c.is_, c.is_)
    if c.P < 64:
        passes = [eighths(rng, shape) for _ in range(c.P)]
    else:
        live = np.array([p for p in range(63) if p not in (5, 17) and not 40 <= p <= 50])
        nb = (c.is_ + 3) // 4
        cls = live[rng.integers(0, len(live), size=(c.B, nb, nb))]
        cls = np.repeat(np.repeat(cls, 4, 1), 4, 2)[:, :c.is_, :c.is_]
        cls[:, : max(2, c.is_ // 5)] = 63
        cls[rng.uniform(size=cls.shape) < 0.1] = -1               # background
        passes = [np.ascontiguousarray(np.broadcast_to((cls == p)[:, None], shape)).astype(np.float32) for p in range(64)]
    grads = [sparse_eighths(rng, shape, c.is_, (0, 2, 3)) for _ in range(c.P)]
    return faces, fi, passes, grads


# ---------------------------------------------------------------------------------------------------------------------------------
# depth (sln_raster_backward_depth)
# ---------------------------------------------------------------------------------------------------------------------------------
Depth = namedtuple("Depth", "name is_ B F")
DEPTH = ([Depth("is%d" % s, s, 1, F_STD) for s in (8, 64, 65, 130, 257)] +
         [Depth("B8-is65", 65, 8, F_STD), Depth("B9-is65", 65, 9, F_STD), Depth("B9-is130", 130, 9, F_STD),
          Depth("B8-F2112", 64, 8, 2112)])


def depth_inputs(c):
    """faces and the oracle's own fi, w, d (near 0.1 as the Renderer's depth mode), grad_depth: seeded normals"""
    from oracle import raster_ref as rr
    faces = batch_geometry(c.is_, c.B, c.F)
    fi, w, d = rr.nmr_forward(faces, c.is_, 0.1, 100.0)
    gd = _rng("depth-" + c.name).standard_normal((c.B, c.is_, c.is_)).astype(np.float32)
    return faces, fi, w, d, gd


# ---------------------------------------------------------------------------------------------------------------------------------
# launcher policy restated (small_batch_split of raster.hip): a change of policy fails the host test instead of un-covering a path
# ---------------------------------------------------------------------------------------------------------------------------------
def small_batch_split(units, max_split, budget=32768):
    s = 1
    while s < max_split and units * s * 2 <= budget:
        s *= 2
    return s


def pixel_map_scan_split(B, F):
    return 1 if B >= 8 else small_batch_split(B * F * 6, 16, 131072)


def depth_bwd_split(B, F):
    return small_batch_split(B * F, 8, 1 << 20) if F <= 2048 else small_batch_split(B * F, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def sum_bound(S, n, share=1.0):
    """|got - g64| <= (8 + 0.5 sqrt(n)) 2^-24 S per element: 8 half-ulps for a term's own roundings (ratio, two products, +eps, a 1-ulp
    reciprocal, a product), 0.5 sqrt(n) for the order of the sum - twice what a serial fp32 sum needs.  share = 0.5: what the
    oracle's own float path has to stay inside."""
    return share * (8.0 + 0.5 * np.sqrt(n.astype(np.float64))) * U * S


# ---------------------------------------------------------------------------------------------------------------------------------
# fused scene pass (sln_scene_forward + sln_scene_backward)
# ---------------------------------------------------------------------------------------------------------------------------------
Scene = namedtuple("Scene", "name is_ B")
SCENE = [Scene("is%d-B%d" % (s, b), s, b) for s in (64, 65, 130) for b in (1, 8, 9)]
SCENE_F = 32
# class 0: wall (the quad); 1: visible, depth channel 0; 2: no visible pixel, depth channel 1 (filled with wall_max); 3: visible,
# no depth channel
SCENE_CHAN = np.array([0, 2, 5, 1], np.int32)
SCENE_DCH = np.array([-1, 0, 1, -1], np.int32)


def scene_geometry(is_, b):
    """faces [32,3,3] and their classes [32]: the set of geometry(is_, b), (g) an object at z = 0.05 - in front of the depth pass's
    near plane 0.1, behind the class passes' 0.001, so the two passes see different winners - faces of class 2 outside the view, and
    faces of class -1 as batch padding"""
    base = geometry(is_, b)
    small = 10 if b % 2 == 0 else 6
    cls = [0, 0] + [1 if (i // 2) % 2 == 0 else 3 for i in range(2 * small)] + [3] + [1, 1]
    if b % 2 == 1:
        cls += [3, 1, 2]                       # (e), the border triangle, the triangle outside the view
    cls += [-1] * (F_STD - len(cls))
    near = _front(np.array([[-0.5, 0.1, 0.05], [-0.1, 0.15, 0.05], [-0.3, 0.6, 0.05]], np.float32))
    faces = list(base) + [near, near[[2, 1, 0]]] + padding(SCENE_F - F_STD - 2)
    cls += [3, 3, 2, 2] + [-1] * (SCENE_F - F_STD - 4)
    assert len(cls) == len(faces) == SCENE_F
    return np.stack(faces).astype(np.float32), np.array(cls, np.int32)


def scene_inputs(c):
    """faces [B,32,3,3], face_class [B,32], grad_final [B,70,is,is]: the class planes in multiples of 3/8 (a third of it, what a
    colour channel receives, is exact) on the thinned pixel set, plane 0 and the depth-hot planes seeded normals.
    Unlike the dense and multi cases the class chain's diffs are NOT exact here: the class-pass value is a sum of trilinear weights
    of an all-ones texture, 1 to within an ulp.  A diff is one rounded product (v_q - v_ref) * g, so its sign - the decision -
    does not depend on a summation order, but it does depend on the forward values being the restatement's."""
    rng = _rng("scene-" + c.name)
    fc = [scene_geometry(c.is_, b) for b in range(c.B)]
    faces, cls = np.stack([f for f, _ in fc]), np.stack([k for _, k in fc])
    g = rng.standard_normal((c.B, 70, c.is_, c.is_)).astype(np.float32)
    g[:, 1:41] = 3.0 * sparse_eighths(rng, (c.B, 40, c.is_, c.is_), c.is_, (0, 2, 3))
    return faces, cls, g
