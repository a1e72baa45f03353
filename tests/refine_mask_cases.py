"""Validity masks of the refinement-loss tests (test_refine_mask_host.py, test_refine_mask_gpu.py): the patterns at the two geometries
the loss kernels distinguish, and a brute-force pooled mask from pool_kernel's index expressions.

  S = 96, sizes (32, 48, 64, 96)   the refinement loop's scales: LDS pooling kernel, separable backward kernel
  S = 40, sizes (8, 12, 16)        P * P = 256 (a multiple of the loss kernel's 128-row blocks), CSR rows of more than 5 entries: the
                                   generic backward kernel
Non-zero = valid, [S, S] uint8 in the row order of the scene tensor's planes."""
import numpy as np

GEOMETRIES = {96: (32, 48, 64, 96), 40: (8, 12, 16)}
PATTERNS = ("ones", "zeros", "corner00", "cornerSS", "interior", "rectangle", "row", "random", "checkerboard")


def pattern(name, S):
    v = np.ones((S, S), np.uint8)
    if name == "ones":
        pass
    elif name == "zeros":
        v[:] = 0
    elif name == "corner00":
        v[0, 0] = 0
    elif name == "cornerSS":
        v[S - 1, S - 1] = 0
    elif name == "interior":
        v[S // 2 + 1, S // 3] = 0
    elif name == "rectangle":
        v[S // 4:S // 2, S // 3:2 * S // 3] = 0
    elif name == "row":
        v[S // 2 + 3, :] = 0
    elif name == "random":
        v[np.random.default_rng(1234 + S).random((S, S)) < 0.05] = 0
    elif name == "checkerboard":
        # (S - 1, S - 1) is invalid: the last pooled pixel of a scale addresses that image pixel alone, four times over
        yy, xx = np.mgrid[0:S, 0:S]
        v = ((yy + xx) % 2 == 1).astype(np.uint8)
    else:
        raise KeyError(name)
    return v


def patterns(S):
    return {name: pattern(name, S) for name in PATTERNS}


def stage_tables(bilinear_taps, S, sizes):
    """(s2_k0, s2_k1 [n_scales, P], s1_i0, s1_i1 [n_scales, pmax]) as RefineLoss._build_tables lays them out, from ``_bilinear_taps``"""
    P, ns, pmax = sizes[-1], len(sizes), max(sizes)
    s2 = [np.zeros((ns, P), np.int64), np.zeros((ns, P), np.int64)]
    s1 = [np.zeros((ns, pmax), np.int64), np.zeros((ns, pmax), np.int64)]
    for k, sz in enumerate(sizes):
        a, b = bilinear_taps(S, sz, True), bilinear_taps(sz, P, False)
        s1[0][k, :sz], s1[1][k, :sz] = a[0], a[1]
        s2[0][k], s2[1][k] = b[0], b[1]
    return s2[0], s2[1], s1[0], s1[1]


def brute_force_valid_pooled(valid, tables, sizes):
    """[n_scales, P, P] bool of one [S, S] mask: pool_kernel's loops (ky / kx in {s2_k0, s2_k1}, yy / xx in {s1_i0, s1_i1}), every one of the
    16 taps looked up, none skipped for its weight"""
    s2_k0, s2_k1, s1_i0, s1_i1 = tables
    P, ns = sizes[-1], len(sizes)
    out = np.ones((ns, P, P), bool)
    oy, ox = np.mgrid[0:P, 0:P]                                  # every pooled pixel of a scale at once; the 16 taps one by one
    for s in range(ns):
        for ky in (s2_k0[s][oy], s2_k1[s][oy]):
            for kx in (s2_k0[s][ox], s2_k1[s][ox]):
                for y in (s1_i0[s][ky], s1_i1[s][ky]):
                    for x in (s1_i0[s][kx], s1_i1[s][kx]):
                        out[s] &= valid[y, x] != 0
    return out
