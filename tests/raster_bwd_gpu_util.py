"""What the per-face GPU tests of the rasterizer (test_raster_bwd_gpu.py, test_raster_texture_chw_gpu.py) share, and what
test_raster_bwd_gpu_helpers_host.py proves about it on the CPU: the operand holder, the host range checks, the comparison with the
double-sum reference, and the float64 restatements of texture sampling and of the projection's adjoint (LAB_NOTES section 25)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

import raster_bwd_cases as rc
from gpu_util import SENT, Dev

GUARD = 64          # floats of SENT on each side of an output


# ---------------------------------------------------------------------------------------------------------------------------------
# operands: held until after the synchronisation, pairwise distinct, index maps in range - all of it before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
class Operands:
    """A thin wrapper of gpu_util.Dev: every operand of a call is uploaded once and kept (CPU tensor and device tensor) for the
    life of the holder, which the caller keeps until after the synchronisation.  `p(name)` is the pointer to pass; `launchable()`
    asserts that no two operands share memory.  upload=False keeps the CPU tensors themselves (the host test of the alias check)."""

    def __init__(self, upload=True):
        self.dev, self.upload = Dev(), upload
        self.t, self.off = {}, {}

    def put(self, name, a, offset_bytes=0):
        assert name not in self.t, name
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        assert t.is_contiguous() and t.dtype in (torch.float32, torch.int32, torch.int64, torch.uint8), (name, t.dtype)
        if self.upload and not t.is_cuda:
            self.dev(t)                              # uploads and keeps both
            self.t[name] = self.dev.m[id(t)][1]
        else:
            self.t[name] = t
        self.off[name] = offset_bytes
        return self.t[name]

    def p(self, name):
        return C.c_void_p(self.t[name].data_ptr() + self.off[name])

    def addr(self, name):
        return self.t[name].data_ptr() + self.off[name]

    def launchable(self):
        spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), k) for k, t in self.t.items())
        ptrs = [s[0] for s in spans]
        assert len(set(ptrs)) == len(ptrs), "operands share a device pointer: %s" % [s[2] for s in spans]
        for (a0, a1, ka), (b0, b1, kb) in zip(spans, spans[1:]):
            assert a1 <= b0, "operands %s and %s overlap" % (ka, kb)
        return self


def check_index_map(name, fi, F):
    """every face index map is an operand: values in [-1, F), anything else is the caller's error (include/sln_hip.h)"""
    fi = np.asarray(fi)
    assert fi.dtype == np.int32, (name, fi.dtype)
    assert fi.size == 0 or (int(fi.min()) >= -1 and int(fi.max()) < F), "%s: index map outside [-1, %d): min %d max %d" % (
        name, F, int(fi.min()), int(fi.max()))


def check_index_list(name, idx, hi, lo=0, exempt=None):
    """face / vertex / class lists in [lo, hi); `exempt`: boolean array of the entries that are out of range on purpose"""
    idx = np.asarray(idx)
    assert idx.dtype == np.int32, (name, idx.dtype)
    ok = (idx >= lo) & (idx < hi)
    if exempt is not None:
        ok = ok | exempt
    assert ok.all(), "%s: %d entries outside [%d, %d)" % (name, int((~ok).sum()), lo, hi)


def guarded(h, name, shape, prefill=None, fill=0.0):
    """an output of `shape` floats with GUARD floats of SENT on each side, held by `h`; the pointer of `name` is the inner one"""
    n = int(np.prod(shape))
    buf = np.full(n + 2 * GUARD, SENT, np.float32)
    buf[GUARD:GUARD + n] = fill if prefill is None else np.asarray(prefill, np.float32).reshape(-1)
    h.put(name, buf, offset_bytes=4 * GUARD)


def read_guarded(h, name, shape):
    n = int(np.prod(shape))
    buf = h.t[name].cpu().numpy()
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all(), "%s: the kernel wrote outside its output" % name
    return buf[GUARD:GUARD + n].reshape(shape).copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def compare(name, got, g64, S, n, split, bound=None, prefill=None, what=("image", "face")):
    """|got - g64| <= bound(S, n) for EVERY element, got == 0 exactly where n == 0, nothing non-finite.  `prefill`: the += contract -
    got is compared with prefill + g64 and the allowance grows by one ulp of |prefill| + |g64|.  Returns the worst err / allowed,
    its place and the largest n."""
    got = np.asarray(got)
    assert got.shape == g64.shape == S.shape == n.shape, (name, got.shape, g64.shape)
    tol = (rc.sum_bound if bound is None else bound)(S, n)
    want = g64
    if prefill is not None:
        pre = np.asarray(prefill, np.float64).reshape(g64.shape)
        want = g64 + pre
        tol = tol + np.spacing((np.abs(pre) + np.abs(g64)).astype(np.float32)).astype(np.float64)
    fin = np.isfinite(got)
    assert fin.all(), "%s [%s]: %d non-finite values, first at %s" % (name, split, int((~fin).sum()), tuple(np.argwhere(~fin)[0]))
    zero = n == 0
    base = 0.0 if prefill is None else np.asarray(prefill, np.float32).reshape(g64.shape)
    nz = zero & (got != base)
    assert not nz.any(), "%s [%s]: %d elements without a term are not exactly %s, first (%s, slot) %s = %r" % (
        name, split, int(nz.sum()), "0" if prefill is None else "the prefill", ", ".join(what), tuple(int(v) for v in np.argwhere(nz)[0]),
        float(got[tuple(np.argwhere(nz)[0])]))
    err = np.abs(got.astype(np.float64) - want)
    bad = np.argwhere(err > tol)
    if bad.shape[0]:
        i = tuple(int(v) for v in bad[np.argmax((err / np.maximum(tol, 1e-300))[tuple(bad.T)])])
        raise AssertionError(
            "%s [%s]: %d of %d elements beyond the bound; worst (%s, slot...) %s: got %.9g want %.9g, n = %d, |g64|/S = %.3g, "
            "error %.1f half-ulps of S (allowed %.1f)" % (
                name, split, bad.shape[0], int((~zero).sum()), ", ".join(what), i, float(got[i]), float(want[i]), int(n[i]),
                abs(g64[i]) / max(S[i], 1e-300), err[i] / max(rc.U * S[i], 1e-300), tol[i] / max(rc.U * S[i], 1e-300)))
    live = ~zero
    if not live.any():
        return 0.0, None, 0
    ratio = np.where(live, err / np.maximum(tol, 1e-300), 0.0)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[w]), tuple(int(v) for v in w), int(n.max())


# ---------------------------------------------------------------------------------------------------------------------------------
# texture sampling, channels first (sln_raster_texture_sample_chw), restated
# ---------------------------------------------------------------------------------------------------------------------------------
# Allowance per output value: TEX_C(ts) * 2^-24 * A * scale with A = sum over the eight cells of |weight * texel|, for textures whose
# texels lie in [0.5, 1] (what the cases use).  Counted from texture_sample_chw_kernel / tex_sample (raster.hip is built without
# contraction, every operation rounds once, at most 2^-24 relative):
#   coordinates: t_k = w_k * (ts - 1) * (depth / z_k) is a quotient and two products, 3 roundings, |dt_k| <= 3 u t_k <= 3 u (ts - 1); the clamp
#     has slope <= 1 and fr_k = t_k - (int)t_k is exact.  The output is linear in fr_k with slope sum over the four cell pairs along
#     axis k of prod_{j != k} wgt_j * (texel_hi - texel_lo): at most max - min of the texels (those weights sum to 1), while
#     A >= min|texel|.  Three axes, (max - min) / min = 1: 3 * 3 (ts - 1) = 9 (ts - 1) - a bound on the movement ACROSS a cell border as
#     well, the interpolant is continuous;
#   weights: 1 - fr rounds once per axis (3) and the product ((1 * a) * b) * c twice: 5;
#   accumulation: the product weight * texel (1) and seven additions onto the first term (7), each below u A: 8;
#   scale: 1.
def TEX_C(ts):
    return 9.0 * (ts - 1) + 14.0


def texture_chw_ref(faces, tex, fi, w, d, ts, eps, scale, dtype=np.float64):
    """Restatement of sln_raster_texture_sample_chw: trilinear sample of cube fi (clamp [0, ts - 1 - eps]), faces >= F_tex = tex.shape[1]
    read cube f - F_tex with texture axes 0 and 2 swapped; output [B, 3, is, is] with rows flipped, times scale; background 0.
    Every operation in `dtype` in the kernel's order.  Returns the image and A * scale (A = sum |weight * texel| per value)."""
    f = dtype
    B, F = faces.shape[:2]
    F_tex, is_ = tex.shape[1], fi.shape[1]
    assert F_tex == F or 2 * F_tex == F
    out = np.zeros((B, 3, is_, is_), f)
    A = np.zeros((B, 3, is_, is_), np.float64)
    for b in range(B):
        ys, xs = np.nonzero(fi[b] >= 0)
        fn = fi[b][ys, xs]
        back = fn >= F_tex
        cube = tex[b][np.where(back, fn - F_tex, fn)].astype(f)               # [n, ts, ts, ts, 3]
        z = faces[b][fn][:, :, 2].astype(f)                                   # [n, 3]
        wk = w[b][ys, xs].astype(f)                                           # [n, 3]
        dep = d[b][ys, xs].astype(f)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (wk * f(ts - 1)) * (dep / z)
        t = np.where(t > 0, t, f(0))                                          # fmaxf(v, 0): NaN gives 0
        t = np.minimum(t, f(np.float32(ts - 1) - np.float32(eps)))
        ti = t.astype(np.int64)
        fr = t - ti.astype(f)
        px = np.zeros((len(fn), 3), f)
        pa = np.zeros((len(fn), 3), np.float64)
        for c in range(8):
            wgt = np.ones(len(fn), f)
            idx = []
            for k in range(3):
                if ((c >> k) & 1) == 0:
                    wgt = wgt * (f(1) - fr[:, k]); idx.append(ti[:, k])
                else:
                    wgt = wgt * fr[:, k]; idx.append(ti[:, k] + 1)
            i0 = np.where(back, idx[2], idx[0]); i2 = np.where(back, idx[0], idx[2])
            texel = cube[np.arange(len(fn)), i0, idx[1], i2]                  # [n, 3]
            px = px + wgt[:, None] * texel
            pa = pa + np.abs(wgt[:, None].astype(np.float64) * texel.astype(np.float64))
        out[b][:, is_ - 1 - ys, xs] = (px * f(scale)).T
        A[b][:, is_ - 1 - ys, xs] = (pa * abs(scale)).T
    return out, A


# ---------------------------------------------------------------------------------------------------------------------------------
# the adjoint of the projection (sln_project_faces_backward), restated per (face, corner) term
# ---------------------------------------------------------------------------------------------------------------------------------
# Allowance per vertex component: (PROJ_C + 0.5 sqrt(n)) * 2^-24 * S.  PROJ_C counts the longest rounding chain of a term of
# project_faces_bwd_kernel (no contraction), each rounding relative to the sum of the absolute values of the products under it:
#   z (and x, y) = p0 R0 + p1 R1 + p2 R2 + t: 3 products + 3 additions = 6;  z + eps: 1;  iz = 1 / (.): 2 (allowing one ulp) -> iz: 9,
#     relative to |iz| * za / |z| (za = the absolute-value form of z: the conditioning of the reciprocal is part of S);
#   gxh = s * (gu K0 - gv K3): products 1, difference 1, s = 2 / os 1, the product by s 1 = 4;
#   gxh * x: 4 + 6 + 1 = 11, + gyh * y: 12;  * iz * iz: 12 + 2 * 9 + 2 = 32;  gz - (.): 33;  * R6k: 34;  the two additions of the
#   three-product sum: 36.  (The gx * Rk path is 4 + 9 + 1 + 1 + 2 = 17.)
PROJ_C = 36.0


def proj_bound(S, n, share=1.0):
    return share * (PROJ_C + 0.5 * np.sqrt(n.astype(np.float64))) * rc.U * S


def project_bwd_ref(verts, faces, K, R, t, os_, eps, gout, dtype=np.float64):
    """Per vertex component of sln_project_faces_backward: g = sum of the (face, corner) terms in `dtype` (serial, corner order), S =
    sum over the terms of the absolute-value form of the term (float64), n = number of terms.  A corner whose vertex index is
    outside [0, V) or whose gout is all zero is no term (both kernels skip it).  Formulas: project_faces_bwd_kernel."""
    f = dtype
    B, V = verts.shape[:2]
    F = faces.shape[1]
    g = np.zeros((B, V, 3), f)
    S = np.zeros((B, V, 3), np.float64)
    n = np.zeros((B, V, 3), np.int64)
    for b in range(B):
        Kb, Rb, tb = K[b].reshape(9).astype(f), R[b].reshape(9).astype(f), t[b].reshape(3).astype(f)
        aK, aR, at = np.abs(Kb).astype(np.float64), np.abs(Rb).astype(np.float64), np.abs(tb).astype(np.float64)
        s = f(2) / f(os_)
        for j in range(3 * F):
            vi = int(faces[b].reshape(-1)[j])
            if vi < 0 or vi >= V:
                continue
            gu, gv, gz = (f(v) for v in gout[b].reshape(-1, 3)[j])
            if gu == 0 and gv == 0 and gz == 0:
                continue
            p = verts[b, vi].astype(f)
            ap = np.abs(p).astype(np.float64)
            x = p[0] * Rb[0] + p[1] * Rb[1] + p[2] * Rb[2] + tb[0]
            y = p[0] * Rb[3] + p[1] * Rb[4] + p[2] * Rb[5] + tb[1]
            z = p[0] * Rb[6] + p[1] * Rb[7] + p[2] * Rb[8] + tb[2]
            xa = ap[0] * aR[0] + ap[1] * aR[1] + ap[2] * aR[2] + at[0]
            ya = ap[0] * aR[3] + ap[1] * aR[4] + ap[2] * aR[5] + at[1]
            za = ap[0] * aR[6] + ap[1] * aR[7] + ap[2] * aR[8] + at[2]
            iz = f(1) / (z + f(eps))
            iza = abs(float(iz)) * za / abs(float(z))
            gxh = s * (gu * Kb[0] - gv * Kb[3])
            gyh = s * (gu * Kb[1] - gv * Kb[4])
            gxa = float(s) * (abs(float(gu)) * aK[0] + abs(float(gv)) * aK[3])
            gya = float(s) * (abs(float(gu)) * aK[1] + abs(float(gv)) * aK[4])
            gx, gy = gxh * iz, gyh * iz
            gzc = gz - (gxh * x + gyh * y) * iz * iz
            gza = abs(float(gz)) + (gxa * xa + gya * ya) * iza * iza
            for k in range(3):
                g[b, vi, k] = g[b, vi, k] + (gx * Rb[k] + gy * Rb[3 + k] + gzc * Rb[6 + k])
                S[b, vi, k] += gxa * iza * aR[k] + gya * iza * aR[3 + k] + gza * aR[6 + k]
                n[b, vi, k] += 1
    return g, S, n


ProjCase = namedtuple("ProjCase", "name F V B")
# n4: the number of 16-byte groups of an image's corner list in project_faces_bwd_det_kernel's four-corner loop (3 F / 4), walked by
# lane l at j = l, l + 128, .. with a second group j + 64 in flight
PROJ = [ProjCase("F%d-B%d" % (F, B), F, V, B) for F, V in ((4, 8),       # n4 = 3: three lanes, no second group
                                                           (5, 9),       # 3 F % 4 != 0: the scalar walk
                                                           (88, 60),     # n4 = 66: lanes 0 and 1 have j2 < n4, the others do not
                                                           (172, 200))   # n4 = 129: lane 0 takes a second loop trip
        for B in (1, 3)]


def proj_inputs(c):
    """verts [B,V,3], faces [B,F,3] int32, K, R [B,3,3], t [B,1,3], gout [B,F,3,3] and `exempt`, the corners whose vertex index is out
    of range on purpose (-1 and V: both kernels skip them).  Vertex V - 1 is referenced by no face; from F = 88 on vertex 0 has a
    degree above 64; a fifth of the corners and one whole face have gout == 0."""
    rng = np.random.default_rng([c.F, c.B, 7])
    verts = rng.uniform(-1, 1, size=(c.B, c.V, 3)).astype(np.float32)
    faces = rng.integers(0, c.V - 1, size=(c.B, c.F, 3)).astype(np.int32)
    exempt = np.zeros(faces.shape, bool)
    if c.F >= 88:
        pick = rng.permutation(3 * c.F)[:70]
        faces.reshape(c.B, -1)[:, pick] = 0
    if c.F >= 5:
        faces[:, 1, 2] = -1; faces[:, c.F - 1, 0] = c.V
        exempt[:, 1, 2] = True; exempt[:, c.F - 1, 0] = True
    gout = rng.standard_normal((c.B, c.F, 3, 3)).astype(np.float32)
    gout[rng.uniform(size=(c.B, c.F, 3)) < 0.2] = 0
    gout[:, c.F // 2] = 0
    K = np.broadcast_to(np.array([[400.0, 0.5, 256.0], [0.25, 410.0, 250.0], [0, 0, 1]], np.float32), (c.B, 3, 3)).copy()
    R = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(c.B)]).astype(np.float32)
    t = np.stack([np.array([[0.1 * b, -0.2, 3.0 + 0.5 * b]], np.float32) for b in range(c.B)])
    return verts, faces, K, R, t, gout, exempt


# ---------------------------------------------------------------------------------------------------------------------------------
# texture cases
# ---------------------------------------------------------------------------------------------------------------------------------
TEX_F = 26           # 25 faces of raster_bwd_cases.geometry and one of padding: F / 2 cubes serve the fill_back form


def tex_inputs(is_, B, ts, half, index_map):
    """faces [B,26,3,3], textures [B, F_tex, ts,ts,ts,3] in [0.5, 1], fi / w / d of the oracle's forward; index_map "random": a map
    uniform in [-1, F) with the weights and depths of the forward (any in-range map is legal)"""
    from oracle import raster_ref as rr
    rng = np.random.default_rng([is_, B, ts, int(half), index_map == "random"])
    faces = rc.batch_geometry(is_, B, TEX_F)
    faces[:, :2, :, :2] *= np.float32(0.625)             # the quad no longer fills the view: background pixels
    fi, w, d = rr.nmr_forward(faces, is_, 0.001, 100.0)
    if index_map == "random":
        fi = rng.integers(-1, TEX_F, size=fi.shape).astype(np.int32)
    F_tex = TEX_F // 2 if half else TEX_F
    tex = rng.uniform(0.5, 1.0, size=(B, F_tex, ts, ts, ts, 3)).astype(np.float32)
    return faces, tex, fi, w, d
