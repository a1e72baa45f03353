"""Confidence images of the refinement-loss tests (test_refine_conf_host.py, test_refine_conf_gpu.py) at the two geometries of
refine_mask_cases.GEOMETRIES, and a brute-force pooled confidence from pool_kernel's index expressions.

Structured patterns: after the 16-tap minimum, uniform random bytes leave a pooled mean of about 12 of 255, which tests little.

  ramp     1 + 254 x / (S - 1) across the columns: every level, no zero
  blocks   8 x 8 blocks at the levels 0 / 64 / 128 / 255 (drawn per block; a tenth of the blocks at 0)
  fused    what a fusion of a few frames leaves: bands at 255 / 128 / 0 (agreed on, seen once, not seen) with 5 % random holes
  binary   refine_mask_cases' rectangle times 255: the validity mask written as a confidence
  full     255 everywhere
  zeros    0 everywhere
[S, S] uint8 in the row order of the scene tensor's planes."""
import numpy as np

import refine_mask_cases as MC

GEOMETRIES = MC.GEOMETRIES
PATTERNS = ("ramp", "blocks", "fused", "binary", "full", "zeros")
GRADED = ("ramp", "blocks", "fused")
BINARY_MASK = "rectangle"


def pattern(name, S):
    if name == "ramp":
        return np.broadcast_to((1 + 254 * np.arange(S) // (S - 1)).astype(np.uint8), (S, S)).copy()
    if name == "blocks":
        nb = (S + 7) // 8
        lv = np.random.default_rng(77 + S).choice(np.array([0, 64, 128, 255], np.uint8), size=(nb, nb), p=[0.1, 0.3, 0.3, 0.3])
        return np.kron(lv, np.ones((8, 8), np.uint8))[:S, :S].copy()
    if name == "fused":
        band = np.array([255, 128, 255, 0, 128, 255], np.uint8)[np.arange(S) * 6 // S]
        c = np.broadcast_to(band[:, None], (S, S)).copy()
        c[np.random.default_rng(4321 + S).random((S, S)) < 0.05] = 0
        return c
    if name == "binary":
        return (MC.pattern(BINARY_MASK, S) * 255).astype(np.uint8)
    if name == "full":
        return np.full((S, S), 255, np.uint8)
    if name == "zeros":
        return np.zeros((S, S), np.uint8)
    raise KeyError(name)


def patterns(S):
    return {name: pattern(name, S) for name in PATTERNS}


def brute_force_conf_pooled(conf, tables, sizes):
    """[n_scales, P, P] uint8 of one [S, S] confidence image: refine_mask_cases.brute_force_valid_pooled's loops with the minimum in the
    place of the AND - every one of the 16 taps looked up, none skipped for its weight"""
    s2_k0, s2_k1, s1_i0, s1_i1 = tables
    P, ns = sizes[-1], len(sizes)
    out = np.full((ns, P, P), 255, np.uint8)
    oy, ox = np.mgrid[0:P, 0:P]
    for s in range(ns):
        for ky in (s2_k0[s][oy], s2_k1[s][oy]):
            for kx in (s2_k0[s][ox], s2_k1[s][ox]):
                for y in (s1_i0[s][ky], s1_i1[s][ky]):
                    for x in (s1_i0[s][kx], s1_i1[s][kx]):
                        out[s] = np.minimum(out[s], conf[y, x])
    return out
