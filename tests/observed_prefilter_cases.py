"""Hand-made source frames for the pre-filter of observed frames (host/reproject.py: prefilter_torch, ObservedPrefilter;
csrc/observed_prefilter.hip): CPU tensors only, built with the helpers and planes of observed_reproject_cases and shared by
test_observed_prefilter_host.py (the torch definition against a plain loop, closed forms and properties) and
test_observed_prefilter_gpu.py (the kernel against the torch definition).

A case is a dict in observed_reproject_cases' layout - ``name``, ``depth_src`` [B, Hs, Ws] float32, ``labels_src`` [B, Hs, Ws] uint8,
``k_src`` [B, 4], ``pose`` [B, 3, 4], ``K_tgt`` [B, 3, 3], ``orig_size``, ``S``, ``near``, ``far``, ``gap``, ``plane`` per frame ((n, c)
or None) - plus ``f``, the factor, and ``k64`` [B, 4], the cameras in float64 as the plane depths were made with.

  identity_2x2_f1      f = 1: a reading keeps its bits, everything else becomes 0.0 with label 0
  blocks_4x4_f2        four blocks: full; a label tie with byte 0; 2 r == n; 2 r < n
  poisoned_5x7_f2      a slanted plane whose remainder row and column hold NaN and byte 255: never read
  plane_9x12_f3        odd factor, a k_out that is no power-of-two fraction of k_src
  front_16x24_f8       the largest block on a fronto-parallel plane: the depth comes back exactly
  speckles_16x24_f8    the largest block: a plane with a speckle nearer and one farther than its block, a block whose majority label
                       belongs to non-members only, a block of two surfaces at exactly half
  holes_37x70_f2       crosses the kernel's tile of 32 x 2 coarse pixels both ways; every kind of pixel without a reading at random,
                       so blocks with r = 0 .. 4; labels from {0, 3, 41, 255}: ties, ties with 0
  plane_37x70_f2       a slanted plane over the same size, for the route
  frames_48x64_f4      B = 3, a k_src per frame: a slanted plane; two front planes with a step of 50 % cut vertically at exactly half a
                       block and, block by block, at every share from none to all; a step of 1 % (one surface) with the bytes 0, 41 and 255
  plane_64x96_f8       a plane large enough for the route at the largest factor
"""
import numpy as np
import torch

import observed_reproject_cases as OC
from conftest import pkg

_CACHE = {}
NAMES = ["identity_2x2_f1", "blocks_4x4_f2", "poisoned_5x7_f2", "plane_9x12_f3", "front_16x24_f8", "speckles_16x24_f8", "holes_37x70_f2", "plane_37x70_f2",
         "frames_48x64_f4", "plane_64x96_f8"]
NEAR_Z, FAR_Z = 2.0, 3.0                                             # the two surfaces of frames_48x64_f4's frame 1, in the source camera
STEP_POSE_TZ = 0.1                                                   # ... which its pose moves along z only


def _case(name, S, f, frames):
    c = OC._case(name, S, frames)
    c["f"] = f
    c["k64"] = np.stack([np.asarray(fr["k"], np.float64) for fr in frames])
    del c["shows"]
    return c


def _frame(rng, Hs, Ws, plane, wide, pose=None, fl=300.0, depth=None):
    return OC._frame(rng, Hs, Ws, plane, pose, fl=fl, depth=depth, k=OC._k_src(Hs, Ws, wide), keep_plane=depth is None)


def _build():
    rng = np.random.default_rng(36)
    nan, inf = np.nan, np.inf
    out = []
    moved = OC._pose(-0.05, 0.1, (0.2, -0.1, 0.3))
    # f = 1
    fr = _frame(rng, 2, 2, OC.FRONT, 0.45, depth=np.array([[1.5, nan], [0.0, 15.0]]))
    fr["labels"] = np.array([[7, 9], [41, 255]], np.uint8)
    out.append(_case("identity_2x2_f1", 16, 1, [fr]))
    # four blocks of 2 x 2
    d = np.full((4, 4), 2.0)
    lab = np.full((4, 4), 5, np.uint8)
    lab[0:2, 2:4] = [[5, 0], [0, 5]]                                 # block (0, 1): two against two, byte 0 wins the tie
    d[2, 0] = nan; d[3, 1] = 0.0                                     # block (1, 0): r = 2 = n / 2, a reading
    d[2, 2] = -1.0; d[2, 3] = inf; d[3, 2] = 15.5                    # block (1, 1): r = 1, no reading
    fr = _frame(rng, 4, 4, OC.FRONT, 0.45, depth=d)
    fr["labels"] = lab
    out.append(_case("blocks_4x4_f2", 16, 2, [fr]))
    # the remainder is poison
    fr = _frame(rng, 5, 7, OC.GENTLE, 1.2)
    fr["depth"][4, :] = nan; fr["depth"][:, 6] = nan
    fr["labels"][4, :] = 255; fr["labels"][:, 6] = 255
    out.append(_case("poisoned_5x7_f2", 16, 2, [fr]))
    # odd factor
    out.append(_case("plane_9x12_f3", 16, 3, [_frame(rng, 9, 12, OC.MILD, 1.2, moved)]))
    out.append(_case("front_16x24_f8", 16, 8, [_frame(rng, 16, 24, OC.FRONT, 0.45)]))
    # blocks of 8 x 8 on 16 x 24: a gentle plane; block (0, 0) a speckle nearer, block (0, 1) one farther, block (1, 0) 33 pixels of
    # the plane with the labels 3 (17 of them) and 4 (16) before 31 pixels of a surface 60 % farther that all say 9, block (1, 1) two
    # surfaces at exactly half: rows 8 .. 11 nearer
    fr = _frame(rng, 16, 24, OC.GENTLE, 1.2)
    fr["labels"][:] = 6
    fr["depth"][3, 5] = 1.0; fr["labels"][3, 5] = 8
    fr["depth"][2, 12] = 6.0; fr["labels"][2, 12] = 8
    blk_d, blk_l = fr["depth"][8:16, 0:8].reshape(-1).copy(), np.zeros(64, np.uint8)
    blk_d[33:] *= 1.6
    blk_l[:17] = 3; blk_l[17:33] = 4; blk_l[33:] = 9
    fr["depth"][8:16, 0:8] = blk_d.reshape(8, 8); fr["labels"][8:16, 0:8] = blk_l.reshape(8, 8)
    fr["depth"][12:16, 8:16] *= 1.5; fr["labels"][8:12, 8:16] = 11; fr["labels"][12:16, 8:16] = 12
    c = _case("speckles_16x24_f8", 16, 8, [fr])
    c["plane"] = [None]
    out.append(c)
    # 37 x 70 at f = 2: 18 x 35 coarse pixels
    fr = _frame(rng, 37, 70, OC.MILD, 0.45)
    kinds = np.array([nan, inf, -inf, 0.0, -0.0, -1.5, 15.5, 16.0, 1e30], np.float32)
    holes = rng.uniform(0, 1, (37, 70)) < 0.35
    fr["depth"][holes] = kinds[rng.integers(0, len(kinds), int(holes.sum()))]
    fr["depth"][20:22, 10:14] = 15.0                                 # the farthest reading
    fr["labels"] = np.array([0, 3, 41, 255], np.uint8)[rng.integers(0, 4, (37, 70))]
    c = _case("holes_37x70_f2", 32, 2, [fr])
    c["plane"] = [None]
    out.append(c)
    out.append(_case("plane_37x70_f2", 32, 2, [_frame(rng, 37, 70, OC.SLANT, 0.45, moved, fl=320.0)]))
    # 48 x 64 at f = 4, three frames with a camera each
    Hs, Ws = 48, 64
    g0 = _frame(rng, Hs, Ws, OC.SLANT, 0.45, OC._pose(0.06, -0.12, (-0.2, 0.1, 0.2)))
    d = np.full((Hs, Ws), NEAR_Z)
    d[:24, 30:] = FAR_Z                                              # columns 28, 29 of block column 7 nearer, 30, 31 farther: half
    for t in range(6 * 16):                                          # rows 24 ..: block t keeps its first t % 17 pixels, column by column
        blk = np.full(16, FAR_Z); blk[:t % 17] = NEAR_Z
        d[24 + 4 * (t // 16):28 + 4 * (t // 16), 4 * (t % 16):4 * (t % 16) + 4] = blk.reshape(4, 4).T
    g1 = _frame(rng, Hs, Ws, OC.FRONT, 0.5, OC._pose(t=(0.05, 0.0, STEP_POSE_TZ)), fl=280.0, depth=d)
    g1["labels"] = np.where(d == NEAR_Z, 21, 22).astype(np.uint8)
    d = np.full((Hs, Ws), 2.0); d[:, 33:] = 2.02
    g2 = _frame(rng, Hs, Ws, OC.FRONT, 0.55, fl=260.0, depth=d)
    g2["labels"][4:8, 4:8] = 0; g2["labels"][8:12, 8:12] = 41; g2["labels"][12:16, 12:16] = 255; g2["labels"][16:20, 16:20] = [[0, 0, 7, 7]] * 4
    out.append(_case("frames_48x64_f4", 16, 4, [g0, g1, g2]))
    # the largest factor, for the route
    out.append(_case("plane_64x96_f8", 16, 8, [_frame(rng, 64, 96, OC.GENTLE, 0.6, OC._pose(0.03, -0.05, (0.1, -0.05, 0.2)), fl=330.0)]))
    return out


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = _build()
    return _CACHE["cases"]


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def filtered(c):
    """``prefilter_torch`` of a case on the host, computed once and never modified: (depth, labels, k_out, counts)"""
    key = (c["name"], "filtered")
    if key not in _CACHE:
        _CACHE[key] = pkg("host.reproject").prefilter_torch(c["depth_src"], c["labels_src"], c["k_src"], c["f"], c["gap"])
    return _CACHE[key]


def coarse(c):
    """the case as observed_reproject_cases.closed_form reads it AFTER the filter: the coarse frames with their cameras"""
    d, l, k, _ = filtered(c)
    return dict(c, depth_src=d, labels_src=l, k_src=k)


def plane_frames():
    """(case, b) of every frame with a plane"""
    return [(c, b) for c in cases() for b, p in enumerate(c["plane"]) if p is not None]


ROUTE_NAMES = ["plane_37x70_f2", "frames_48x64_f4", "plane_64x96_f8"]


def torch_route(c, dtype):
    """``reproject_torch(prefilter=f)`` of a case with the rasterizer's C restatement, once per (case, dtype)"""
    return OC.torch_route(c, dtype, prefilter=c["f"])


def junk(B, Hd, Wd, device="cpu"):
    """the four outputs, pre-filled with values no result holds"""
    return OC.junk(dict(depth=(B, Hd, Wd), labels=(B, Hd, Wd), k_out=(B, 4), counts=(B, 3)), device)
