"""Hand-made source frames for the reprojection of observed frames (host/reproject.py, csrc/observed_reproject.hip): CPU tensors only,
shared by test_observed_reproject_host.py (the torch definition against closed forms and brute force) and test_observed_reproject_gpu.py
(the kernels against the torch definition).  Frames of 2 x 2 (one cell), 3 x 5, 18 x 34 (one vertex past the kernel's 16 x 16 tile of
cells both ways) and 48 x 64 pixels; targets of S = 16, 32 and 64; B = 1 and 3 with a camera and a pose of its own per frame; principal
points off the grid.

A case is a dict: ``name``, ``depth_src`` [B, Hs, Ws] float32, ``labels_src`` [B, Hs, Ws] uint8, ``k_src`` [B, 4], ``pose`` [B, 3, 4],
``K_tgt`` [B, 3, 3], ``orig_size``, ``S``, ``near``, ``far``, ``gap``, and per frame ``plane`` ((n, c): the surface n . p = c in source
camera coordinates, in float64, or None) and ``shows`` (True: the frame is meant to show a surface - the float64 route must hit a
quarter of the target; False: it is meant to show nothing; None: neither is claimed).
"""
import numpy as np
import torch

from conftest import pkg

ORIG = 512.0
NEAR, FAR, GAP = 0.1, 100.0, 0.05
_CACHE = {}


def _rot(ax, ay):
    """R_y(ay) . R_x(ax), float64"""
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return ry @ rx


def _k_src(Hs, Ws, wide=0.45):
    """a wide source camera with non-square pixels and a principal point off the grid"""
    return np.array([wide * Ws, wide * Hs, Ws / 2 + 0.3, Hs / 2 - 0.2])


def _k_tgt(fl, dx=0.0, dy=0.0):
    return np.array([[fl, 0, ORIG / 2 + dx], [0, fl, ORIG / 2 + dy], [0, 0, 1.0]])


def _pose(ax=0.0, ay=0.0, t=(0.0, 0.0, 0.0)):
    return np.concatenate([_rot(ax, ay), np.asarray(t, np.float64)[:, None]], 1)


def _plane_depth(Hs, Ws, k, n, c):
    """the depth image of the plane n . p = c under k = (fx, fy, cx, cy), float64"""
    u, v = np.arange(Ws) + 0.5, np.arange(Hs) + 0.5
    rx, ry = (u[None, :] - k[2]) / k[0], (v[:, None] - k[3]) / k[1]
    return c / (n[0] * rx + n[1] * ry + n[2])


def _labels(rng, Hs, Ws):
    """class bytes 1 .. 40 in blocks of 2 x 3 pixels: neighbours differ, so the nearest-pixel rule shows"""
    blocks = rng.integers(1, 41, ((Hs + 1) // 2, (Ws + 2) // 3))
    return np.repeat(np.repeat(blocks, 2, 0), 3, 1)[:Hs, :Ws].astype(np.uint8)


FRONT = (np.array([0.0, 0.0, 1.0]), 2.0)
# (slopes chosen so that the depths of a cell differ by less than half the gap at every frame size they are used at)
SLANT = (np.array([0.15, -0.1, 1.0]), 3.0)
MILD = (np.array([0.1, -0.06, 1.0]), 3.0)
GENTLE = (np.array([0.02, -0.015, 1.0]), 2.5)


def _frame(rng, Hs, Ws, plane=FRONT, pose=None, fl=300.0, shows=True, depth=None, k=None, keep_plane=True, k_given=None):
    k = _k_src(Hs, Ws) if k is None else k
    d = _plane_depth(Hs, Ws, k, *plane) if depth is None else depth
    k = k if k_given is None else k_given                           # (the depths are those of a sound camera either way)
    return dict(depth=d.astype(np.float32), labels=_labels(rng, Hs, Ws), k=k, pose=_pose() if pose is None else pose,
                K=_k_tgt(fl, dx=rng.uniform(-6, 6), dy=rng.uniform(-6, 6)), plane=plane if keep_plane else None, shows=shows)


def _case(name, S, frames):
    f32 = lambda key: torch.from_numpy(np.stack([np.asarray(f[key], np.float64) for f in frames]).astype(np.float32))
    return dict(name=name, S=S, orig_size=ORIG, near=NEAR, far=FAR, gap=GAP,
                depth_src=torch.from_numpy(np.stack([f["depth"] for f in frames])), labels_src=torch.from_numpy(np.stack([f["labels"] for f in frames])),
                k_src=f32("k"), pose=f32("pose"), K_tgt=f32("K"), plane=[f["plane"] for f in frames], shows=[f["shows"] for f in frames])


def _build():
    rng = np.random.default_rng(20)
    out = []
    moved = _pose(-0.05, 0.1, (0.2, -0.1, 0.3))
    # one cell, a fronto-parallel plane, a translated target
    out.append(_case("one_cell_2x2_s16", 16, [_frame(rng, 2, 2, FRONT, _pose(t=(0.1, -0.05, 0.2)), fl=420.0)]))
    # 3 x 5, a slanted plane seen from a rotated and translated target
    out.append(_case("slanted_3x5_s16", 16, [_frame(rng, 3, 5, GENTLE, moved, fl=380.0)]))
    # 18 x 34: one vertex past the tile both ways.  Frame 0 a fronto-parallel plane; frame 1 two planes with a step well above the gap
    # (2 against 3) and one well below it (2 against 2.02); frame 2 a slanted plane with every kind of pixel without a reading and the
    # label bytes 0, 41 and 255
    Hs, Ws = 18, 34
    f0 = _frame(rng, Hs, Ws, FRONT, _pose(0.04, -0.08, (-0.15, 0.1, 0.25)))
    d = np.full((Hs, Ws), 2.0); d[:, 20:] = 3.0; d[10:, :20] = 2.02
    f1 = _frame(rng, Hs, Ws, FRONT, _pose(t=(0.05, 0.0, 0.1)), depth=d, keep_plane=False, fl=280.0)
    f2 = _frame(rng, Hs, Ws, MILD, moved, fl=320.0)
    for (i, j), v in zip(((2, 3), (5, 9), (8, 15), (11, 21), (14, 27), (16, 33), (0, 0)), (np.nan, np.inf, 0.0, -1.5, 15.5, -np.inf, 16.0)):
        f2["depth"][i, j] = np.float32(v)
    f2["labels"][3, 3:6] = (0, 41, 255); f2["labels"][9, 12:18] = 0; f2["labels"][12, 20] = 41; f2["labels"][15, 30] = 255
    out.append(_case("tile_edge_18x34_s32", 32, [f0, f1, f2]))
    # 48 x 64.  Frame 0 a slanted plane from a rotated target; frame 1 the same surface seen from behind (the target stands behind the
    # plane and looks back at the source); frame 2 a fronto-parallel surface with a patch 2 % nearer (no step) under a pose that leaves
    # the surface at z = 0.12 and the patch at 0.08: the cells on the patch's rim have one, two or three corners inside `near`
    Hs, Ws = 48, 64
    g0 = _frame(rng, Hs, Ws, SLANT, _pose(0.06, -0.12, (-0.2, 0.1, 0.2)), fl=300.0)
    behind = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.array([[0.0], [0.0], [6.0]])], 1)
    g1 = _frame(rng, Hs, Ws, SLANT, behind, shows=False)
    d = np.full((Hs, Ws), 2.0); d[10:24, 20:33] = 1.96
    g2 = _frame(rng, Hs, Ws, FRONT, _pose(t=(0.01, -0.005, -1.88)), depth=d, keep_plane=False, fl=260.0, shows=None)
    out.append(_case("frames_48x64_s64", 64, [g0, g1, g2]))
    # frames that show nothing: no reading anywhere; a frame with fx = 0 and one with fy < 0 - and a sound frame beside them
    Hs, Ws = 3, 5
    h0 = _frame(rng, Hs, Ws, FRONT, shows=False, keep_plane=False,
                depth=np.array([[np.nan, 0.0, -1.0, 15.5, np.inf], [0.0, -0.0, -np.inf, 1e30, np.nan], [16.0, -1e-30, 0.0, np.nan, 100.0]]))
    bad = _k_src(Hs, Ws); bad[0] = 0.0
    h1 = _frame(rng, Hs, Ws, FRONT, shows=False, k_given=bad, keep_plane=False)
    h2 = _frame(rng, Hs, Ws, FRONT, _pose(t=(0.0, 0.0, 0.1)), fl=400.0)
    out.append(_case("nothing_to_show_3x5_s16", 16, [h0, h1, h2]))
    neg = _k_src(Hs, Ws); neg[1] = -neg[1]
    out.append(_case("negative_fy_3x5_s16", 16, [_frame(rng, Hs, Ws, FRONT, shows=False, k_given=neg, keep_plane=False)]))
    return out


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = _build()
    return _CACHE["cases"]


NAMES = ["one_cell_2x2_s16", "slanted_3x5_s16", "tile_edge_18x34_s32", "frames_48x64_s64", "nothing_to_show_3x5_s16", "negative_fy_3x5_s16"]


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def torch_route(c, dtype, route="reproject_torch", **more):
    """host/reproject.py's ``route`` (``reproject_torch``, ``reproject_views_torch``) of a case of this module's layout, of
    observed_fuse_cases' or of observed_prefilter_cases', with the rasterizer's C restatement: computed once per (route, case, dtype)
    and never modified"""
    key = (route, c["name"], dtype)
    if key not in _CACHE:
        from oracle import raster_ref
        fn = getattr(pkg("host.reproject"), route)
        _CACHE[key] = fn(c["depth_src"], c["labels_src"], c["k_src"], c["pose"], c["K_tgt"], c["orig_size"], c["S"], raster_ref.nmr_forward,
                         near=c["near"], far=c["far"], gap=c["gap"], dtype=dtype, **more)
    return _CACHE[key]


# outputs pre-filled with values no result holds, by the name of the output: (value, dtype)
JUNK = dict(depth=(7.5, torch.float32), labels=(9, torch.uint8), source=(201, torch.uint8), count=(202, torch.uint8), agree=(203, torch.uint8),
            hits=(-3, torch.int64), wins=(-5, torch.int64), k_out=(-2.5, torch.float32), counts=(-3, torch.int64))


def junk(shapes, device="cpu"):
    """name -> shape: a tensor per output, filled with its value of ``JUNK``"""
    return {k: torch.full(tuple(s), JUNK[k][0], dtype=JUNK[k][1], device=device) for k, s in shapes.items()}


def face_error(got, want):
    """largest |got - want| / max(1, |want|) over the slots that both keep, and the number of slots only one of them collapsed"""
    got, want = got.double(), want.double()
    dead_g, dead_w = (got == 0).all(-1).all(-1), (want == 0).all(-1).all(-1)
    both = ~dead_g & ~dead_w
    err = ((got - want).abs() / want.abs().clamp(min=1.0))[both]
    return (float(err.max()) if err.numel() else 0.0), int((dead_g != dead_w).sum())


def closed_form(c, b):
    """Frame b of a plane case: the depth of the plane along the ray of every target pixel centre, in float64 from the float32 camera
    parameters the routes read, in the planes' row order -> (depth [S, S], inside [S, S], us, vs): ``inside`` marks the pixels whose
    source position (us, vs) - in source pixels, centres at .5 - lies a full source pixel inside the grid (and whose surface point is a
    reading in front of both cameras)."""
    n, cc = c["plane"][b]
    S, os_ = c["S"], c["orig_size"]
    K, P, k = c["K_tgt"][b].double().numpy(), c["pose"][b].double().numpy(), c["k_src"][b].double().numpy()
    Hs, Ws = c["depth_src"].shape[1:]
    col, row = np.meshgrid(np.arange(S) + 0.5, np.arange(S) + 0.5)
    xh, yh = (os_ * col / S - K[0, 2]) / K[0, 0], (os_ * row / S - K[1, 2]) / K[1, 1]
    R, t = P[:, :3], P[:, 3]
    m = R @ n
    z = (cc + m @ t) / (m[0] * xh + m[1] * yh + m[2])
    pt = np.stack((xh * z, yh * z, z), -1)
    ps = (pt - t) @ R                                                 # R^T (p_t - t)
    us, vs = k[0] * ps[..., 0] / ps[..., 2] + k[2], k[1] * ps[..., 1] / ps[..., 2] + k[3]
    inside = (us >= 1.5) & (us <= Ws - 1.5) & (vs >= 1.5) & (vs <= Hs - 1.5) & (ps[..., 2] > 0) & (ps[..., 2] <= 15) & (z > 2 * c["near"])
    return torch.from_numpy(z), torch.from_numpy(inside), torch.from_numpy(us), torch.from_numpy(vs)


def raster_bound(c, faces64, b):
    """What the float32 rasterizer may add to the depth of frame b's plane, from its own arithmetic (oracle/raster_ref.cpp): a
    barycentric weight is (a x + b y + c) / den in PIXEL coordinates below S; c is a difference of two products of such coordinates,
    each rounded by up to 2^-24 S^2, and a, b, den and the sum are rounded again - an absolute error of at most 16 * 2^-24 * S^2 / den
    per weight, den twice the face's area in pixels.  The interpolated depth moves by at most that times the spread of z over the face;
    the reciprocals and the final rounding add a few units of 2^-24 z.  The corners themselves reach the rasterizer as float32: 2^-24 in
    NDC, S / 2 times that in pixels, which moves depth by the face's slope - inside the same term.  -> the largest such sum over the
    kept faces of the frame."""
    f = faces64[b].double()
    keep = ~(f == 0).all(-1).all(-1)
    if not bool(keep.any()):
        return 0.0
    f = f[keep]
    S = c["S"]
    px = (f[..., :2] * S + S - 1) * 0.5
    den = ((px[:, 1, 0] - px[:, 0, 0]) * (px[:, 2, 1] - px[:, 0, 1]) - (px[:, 1, 1] - px[:, 0, 1]) * (px[:, 2, 0] - px[:, 0, 0])).abs()
    spread = f[..., 2].max(-1).values - f[..., 2].min(-1).values
    zmax = f[..., 2].max()
    u = 2.0 ** -24
    return float((16 * u * S * S / den * spread).max() + 8 * u * zmax)


# ------------------------------------------------------------------------------------------------------------------------------
# the round trip of a render: a scene tensor's own planes as a source frame of their own camera
# ------------------------------------------------------------------------------------------------------------------------------
ROUND_TRIP_S = 64
ROUND_TRIP_SEED = 11


def round_trip_inputs(room_box, S, B=1):
    """(k_src [B, 4], pose [B, 3, 4], K_tgt [B, 3, 3], orig_size) of the identity round trip for a room row, CPU float32"""
    RP = pkg("host.reproject")
    K, _, _, orig = RP.refine_view(room_box, S)
    eye = torch.cat((torch.eye(3), torch.zeros(3, 1)), 1)
    return RP.scene_as_source(K, orig, S)[None].repeat(B, 1), eye[None].repeat(B, 1, 1).contiguous(), K[None].repeat(B, 1, 1).contiguous(), orig


def settled(depth, labels, gap=GAP):
    """[B, S, S] bool: the pixels whose 3 x 3 neighbourhood holds only readings, no depth step above ``gap`` - a step being what the
    definition calls one: none of the eight slots of the four cells round the pixel has dmax - dmin > gap * dmin (float32) - and one
    label: where a round trip has nothing to decide.  Border pixels have no such neighbourhood."""
    import torch.nn.functional as Fn
    d = depth.float()
    reading = (d > 0) & (d <= 15.0)
    a, b, c, dd = d[:, :-1, :-1], d[:, 1:, :-1], d[:, :-1, 1:], d[:, 1:, 1:]
    g = torch.tensor(gap, dtype=torch.float32)

    def one_surface(p, q, r):
        lo, hi = torch.minimum(p, torch.minimum(q, r)), torch.maximum(p, torch.maximum(q, r))
        return ~((hi - lo) > g * lo)
    cell = one_surface(a, b, c) & one_surface(dd, c, b)                                           # [B, S - 1, S - 1]
    cells = -Fn.max_pool2d(-cell.float()[:, None], 2, stride=1)[:, 0] > 0                       # the four cells round an inner pixel
    every = -Fn.max_pool2d(-reading.float()[:, None], 3, stride=1)[:, 0] > 0
    lab = labels.float()[:, None]
    one = Fn.max_pool2d(lab, 3, stride=1)[:, 0] == -Fn.max_pool2d(-lab, 3, stride=1)[:, 0]
    out = torch.zeros_like(reading)
    out[:, 1:-1, 1:-1] = cells & every & one
    return out
