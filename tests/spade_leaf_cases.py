"""Case tables, seeded inputs and reference results of the SPADE leaf-kernel tests, shared by tests/test_spade_leaf_gpu.py (the
kernels of csrc/spade.hip through the C ABI) and tests/test_spade_leaf_ref_host.py (the yardstick alone must stay inside the cap).
torch and numpy only; the library is never imported here.

evaluate(family, case) -> (inputs: dict of CPU tensors, refs: dict name -> (fp64 result, fp32-path result)).

Tolerance (parity.assert_close_conditioned with rtol = 2^-23, k = 8):
    |got - ref64| <= ATOL + 2^-23 * max|ref64| + 8 * max|ref32 - ref64|
one fp32 ulp at the tensor's magnitude plus eight times the fp32 evaluation's own distance from fp64.  CAP: the allowed error of
every case must stay at or below 1e-5 of the tensor's maximum, or the inputs are badly chosen.
"""
import zlib

import numpy as np
import torch

import spade_leaf_ref as R

D64, D32 = torch.float64, torch.float32
ULP32 = 2.0 ** -23
K_NOISE = 8.0            # parity.assert_close_conditioned's default
ATOL = 1e-30             # all-zero tensors only
CAP = 1e-5
EPS = 1e-5
ND = 16                  # depth features of SPADE4 (NHIDDEN / 8)
SENT = -777.25


def allowed(r64, r32):
    """-> (allowed max error, scale = max |ref64|)"""
    r64 = np.asarray(r64, np.float64); r32 = np.asarray(r32, np.float64)
    scale = float(max(np.abs(r64).max(), 1e-30)) if r64.size else 1.0
    noise = float(np.abs(r32 - r64).max()) if r64.size else 0.0
    return ATOL + ULP32 * scale + K_NOISE * noise, scale


def _gen(family, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((family,) + tuple(case)).encode()))


def _both(fn):
    return fn(D64), fn(D32)


# ------------------------------------------------------------------------------------------------ tables
# (Hi, Wi, Ho, Wo, BC).  26 -> 22 and 39 -> 33 tell the float rule from dst * in // out (test_spade_leaf_ref_host.py)
RESIZE_NEAREST = [s + (bc,) for s in [(26, 39, 22, 33), (39, 26, 33, 22), (256, 256, 8, 8), (8, 8, 16, 16), (1, 1, 4, 4), (7, 5, 10, 9)]
                  for bc in (1, 6)]
RESIZE_BILINEAR = [s + (bc,) for s in [(7, 5, 10, 9), (10, 14, 7, 20), (20, 20, 14, 14), (3, 1, 6, 2), (256, 256, 8, 8), (250, 250, 177, 177)]
                   for bc in (1, 6)]
# (H, W, mode, BC)
UPSAMPLE = [(h, w, m, bc) for (h, w) in [(1, 1), (1, 4), (3, 5), (8, 8)] for m in (0, 1) for bc in (1, 5)]
# (Cs, H, W, B)
DEPTH_CONCAT = [(41, 2, 3, 1), (41, 17, 19, 2), (1, 8, 8, 2), (41, 16, 16, 3)]
# (B, n, kind).  n <= 4096: one workgroup per sample; 4097: two; 40 * 64 * 64: 40; 40 * 128 * 128: the 128-workgroup cap, the loop
# strides; B = 65: a second finalize workgroup.  cond: 50 + 0.01 randn (the one-pass formula needs its fp64 sums); const: var clamps
N_MID, N_BIG = 40 * 64 * 64, 40 * 128 * 128
LN_STATS = [(1, 2, "randn"), (1, 231, "randn"), (1, 4096, "randn"), (1, 4097, "randn"), (1, N_MID, "randn"), (1, N_BIG, "randn"),
            (3, 2, "randn"), (3, 231, "randn"), (3, 4097, "randn"), (3, N_MID, "randn"), (65, 231, "randn"),
            (3, N_MID, "cond"), (1, N_BIG, "cond"), (2, 4096, "const")]
LN_STATS_DET = (1, N_BIG, "randn")
# (B, rep)
LN_FINALIZE = [(1, 1), (1, 4), (65, 1), (65, 4)]
# (C, hw), B = 2.  C / 8 = 1, 3 (scalar w2 path), 32 (vector path), 33 (scalar, second hidden-row iteration), 128 (vector)
SE = [(c, hw) for c in (8, 24, 256, 264, 1024) for hw in (1, 100, 4096)]
SE_B = 2
# (B, C, H, W, up_mode, xs_up, with_sums, with_stats, kind)
TAIL_PHASES = [(b, c, 4, 4, -1, 0, s, 1, "randn") for s in (1, 0) for (b, c) in [(1, 256), (1, 264), (2, 1024)]] + \
              [(9, 264, 4, 4, -1, 0, 1, 1, "randn")]
TAIL_NARROW = [(2, 8, 2, 2, m, u, 0, 1, "randn") for m in (0, 1) for u in (0, 1)] + \
              [(2, 8, 2, 4, m, u, 0, 1, "randn") for m in (-1, 0, 1) for u in (0, 1)] + \
              [(2, 8, 1, 4, m, 0, 0, 1, "randn") for m in (-1, 0, 1)] + \
              [(2, 8, 6, 6, m, u, 0, 1, "randn") for m in (0, 1) for u in (0, 1)]
# 512 workgroups per sample with statistics; 4096 / B without.  (1, 16, 128, 128) bilinear: the two-row form has C (H + 1) W / 2 items,
# and only there do 512 workgroups leave its loop a second iteration
TAIL_STRIDED = [(1, 40, 64, 64, 0, 0, 0, 1, "randn"), (1, 40, 64, 64, 1, 0, 0, 1, "randn"), (16, 72, 32, 32, 1, 0, 0, 0, "randn"),
                (1, 16, 128, 128, 1, 0, 0, 1, "randn")]
# n = 32 * 64 * 64 per sample: the fp32 rounding of the outputs (one ulp of 75 = 7.6e-6 under a spread of 0.011) moves the sample
# variance by its chance correlation with the values, ~ 1 / sqrt(n) - at 16 x 16 x 16 elements that alone is 2e-5 of 1 / (std + eps)
TAIL_COND = [(2, 32, 64, 64, -1, 0, 0, 1, "cond")]
TAIL = TAIL_PHASES + TAIL_NARROW + TAIL_STRIDED + TAIL_COND
# (C, H, W, x_up, act), B = 3
APPLY = [(c, h, w, u, a) for c in (8, 40, 100) for (h, w, u) in [(2, 6, 0), (10, 10, 0), (4, 4, 1), (8, 12, 1)] for a in (0, 2)]
APPLY_B = 3
# (C, H, W, xin_up, act), Cin = 128, B = 2
MODULATE = [(c, h, w, u, a) for c in (8, 40, 100) for (h, w) in [(8, 8), (4, 12)] for u in (0, 1) for a in (0, 2)]
MOD_CIN, MOD_B = 128, 2

FAMILIES = {"resize_nearest": RESIZE_NEAREST, "resize_bilinear": RESIZE_BILINEAR, "upsample2x": UPSAMPLE, "depth_concat": DEPTH_CONCAT,
            "ln_stats": LN_STATS, "ln_finalize": LN_FINALIZE, "se_scale_add": SE, "block_tail": TAIL, "spade_apply": APPLY,
            "modulate": MODULATE}


# ------------------------------------------------------------------------------------------------ inputs and references
def _se_weights(g, C, gap, spread=2.0):
    """w0 ~ randn / sqrt(C), w2 ~ randn / sqrt(Cr), then fitted to the pool values `gap` [B, C] of the case: a hidden row that is
    negative for every sample is negated (it would switch the block off; C = 8 has one row), and w2 is scaled so that the logits have
    standard deviation `spread` - they spread over several units and the logistic is not saturated."""
    Cr = C // 8
    w0, w2 = torch.randn(Cr, C, generator=g) / C ** 0.5, torch.randn(C, Cr, generator=g) / Cr ** 0.5
    dead = ((gap.double() @ w0.double().t()) <= 0).all(0)
    w0[dead] = -w0[dead]
    logits = (gap.double() @ w0.double().t()).clamp_min(0) @ w2.double().t()
    return w0, (w2 * (spread / float(logits.std()))).contiguous()


def _channel_data(g, B, C, H, W):
    """randn with a per-channel mean of spread 1 (what the average pool sees) and an offset (the LayerNorm mean is not ~0)"""
    return torch.randn(B, C, H, W, generator=g) + torch.randn(B, C, 1, 1, generator=g) + 0.2


def _ev_resize(case, mode):
    Hi, Wi, Ho, Wo, BC = case
    src = torch.randn(BC, Hi, Wi, generator=_gen("resize%d" % mode, case))
    if mode == 1:
        # The source coordinate (dst + 0.5) * in / out - 0.5 is an fp32 number of magnitude up to `in`: its two roundings move the
        # blend weight by ~1.2e-7 * in, and the result by that times the difference of the two neighbours.  White noise of unit
        # spread would put eight times that above the cap from in = 20 on; an offset of 2 under noise of spread 2 / in keeps it inside
        # at every size, and a wrong weight or a neighbour one pixel off still shows as ~1e-3 .. 1e-1 of the maximum.
        src = 2.0 + min(1.0, 2.0 / max(Hi, Wi)) * src
    return dict(src=src), {"out": _both(lambda d: R.resize(src, Ho, Wo, mode, d))}


def _ev_upsample(case):
    H, W, mode, BC = case
    x = torch.randn(BC, H, W, generator=_gen("upsample2x", case))
    return dict(x=x), {"out": _both(lambda d: R.upsample2x(x, mode, d))}


def _ev_depth_concat(case):
    Cs, H, W, B = case
    g = _gen("depth_concat", case)
    seg = torch.rand(B, Cs, H, W, generator=g) * 2 - 1
    wpd = torch.randn(ND, 9, generator=g) / 3
    bpd = torch.randn(ND, generator=g) * 0.1
    return dict(seg=seg, wpd=wpd, bpd=bpd), {"out": _both(lambda d: R.depth_concat(seg, wpd, bpd, ND, d))}


def ln_input(case):
    B, n, kind = case
    g = _gen("ln_stats", case)
    if kind == "const":
        return torch.tensor([1.5, -3.25, 0.75])[:B].view(B, 1).expand(B, n).contiguous()      # every partial sum is exact in fp64
    if kind == "cond":
        return 50.0 + 0.01 * torch.randn(B, n, generator=g)
    return torch.randn(B, n, generator=g) * 1.5 + 0.7


def _split_stats(pair):
    (a, b) = pair
    return {"mean": (a[:, 0], b[:, 0]), "inv": (a[:, 1], b[:, 1])}


def _ev_ln_stats(case):
    B, n, kind = case
    x = ln_input(case)
    if kind == "const":      # var clamps at 0: held to what the fp64 one-pass formula gives from exact sums
        s, q = x.double().sum(1), (x.double() ** 2).sum(1)
        return dict(x=x), _split_stats(_both(lambda d: R.ln_finalize(s, q, n, 1, EPS, d)))
    return dict(x=x), _split_stats(_both(lambda d: R.ln_stats(x, EPS, d)))


def _ev_ln_finalize(case):
    B, rep = case
    x = torch.randn(B, 3, 4, 5, generator=_gen("ln_finalize", case)) * 1.5 + 0.7
    flat = x.double().reshape(B, -1)
    return dict(x=x, s=flat.sum(1), q=(flat * flat).sum(1), n_acc=flat.shape[1]), _split_stats(_both(lambda d: R.ln_stats(x, EPS, d, rep)))


def _ev_se(case):
    C, hw = case
    g = _gen("se_scale_add", case)
    dx = _channel_data(g, SE_B, C, hw, 1)
    xs = torch.randn(SE_B, C, hw, 1, generator=g) + 0.3
    w0, w2 = _se_weights(g, C, dx.double().mean((2, 3)))
    o64, s64 = R.se_scale_add(xs, dx, w0, w2, D64)
    o32, s32 = R.se_scale_add(xs, dx, w0, w2, D32)
    return dict(xs=xs, dx=dx, w0=w0, w2=w2), {"scale": (s64, s32), "out": (o64, o32)}


def _ev_tail(case):
    B, C, H, W, up_mode, xs_up, with_sums, with_stats, kind = case
    g = _gen("block_tail", case)
    hs, ws = (H // 2, W // 2) if xs_up else (H, W)
    if kind == "cond":       # out = 50 + 50 scale + O(0.01): the SE block all but switched off, or the channels' scales set the spread
        dx = 50.0 + 0.01 * torch.randn(B, C, H, W, generator=g)
        xs = 50.0 + 0.01 * torch.randn(B, C, hs, ws, generator=g)
        w0, w2 = _se_weights(g, C, dx.double().mean((2, 3)), spread=1e-6)
    else:
        dx = _channel_data(g, B, C, H, W)
        xs = torch.randn(B, C, hs, ws, generator=g) + 0.3
        w0, w2 = _se_weights(g, C, dx.double().mean((2, 3)))
    sums = dx.double().sum((2, 3)).contiguous()
    inp = dict(xs=xs, dx=dx, w0=w0, w2=w2, sums=sums if with_sums else None)
    sc = _both(lambda d: R.se_scale(sums if with_sums else dx, H * W, w0, w2, d))
    refs = {"scale": sc}
    r = [R.block_tail(xs, xs_up, dx, sc[i], up_mode, d, 1, EPS) for i, d in enumerate((D64, D32))]
    refs["out"] = (r[0][0], r[1][0])
    if with_stats:
        for rep in (1, 4):
            st = (r[0][1], r[1][1]) if rep == 1 else (R.ln_stats(r[0][0], EPS, D64, 4), R.ln_stats(r[1][0], EPS, D32, 4))
            for k, v in _split_stats(st).items():
                refs["%s_rep%d" % (k, rep)] = v
    return inp, refs


def rows_pad_of(C):
    return 64 * ((C + 31) // 32)


def _stats_of(x, up):
    """what the statistics kernel hands the modulation: fp32 (mean, 1 / (std + eps)) of the tensor that is normalised"""
    return R.ln_stats(x, EPS, D32, 4 if up else 1).contiguous()


def _ev_apply(case):
    C, H, W, x_up, act = case
    g = _gen("spade_apply", case)
    hs, ws = (H // 2, W // 2) if x_up else (H, W)
    x = (torch.randn(APPLY_B, C, hs, ws, generator=g) * 2 + 0.5) * torch.arange(1, APPLY_B + 1).view(-1, 1, 1, 1)      # distinct statistics
    rp = rows_pad_of(C)
    gb = torch.full((rp, H, W), float("nan"))          # rows of no channel: NaN, never read
    rg, rb = R.packed_rows(C)
    gb[rg] = torch.randn(C, H, W, generator=g) * 0.5
    gb[rb] = torch.randn(C, H, W, generator=g)
    stats = _stats_of(x, x_up)
    return dict(x=x, gb=gb, stats=stats, rows_pad=rp), {"out": _both(lambda d: R.spade_apply(x, x_up, gb, stats, C, act, 0.2, d))}


def _ev_modulate(case):
    C, H, W, xin_up, act = case
    g = _gen("modulate", case)
    B, Cin = MOD_B, MOD_CIN
    actv = torch.relu(torch.randn(B, Cin, H, W, generator=g))
    hs, ws = (H // 2, W // 2) if xin_up else (H, W)
    xin = (torch.randn(B, C, hs, ws, generator=g) * 2 + 0.5) * torch.arange(1, B + 1).view(-1, 1, 1, 1)
    wg = torch.randn(C, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5; bg = torch.randn(C, generator=g) * 0.1
    wb = torch.randn(C, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5; bb = torch.randn(C, generator=g) * 0.1
    stats = _stats_of(xin, xin_up)
    return dict(actv=actv, xin=xin, wg=wg, bg=bg, wb=wb, bb=bb, stats=stats), \
        {"out": _both(lambda d: R.modulate(actv, wg, bg, wb, bb, xin, xin_up, stats, act, 0.2, d))}


_EVAL = {"resize_nearest": lambda c: _ev_resize(c, 0), "resize_bilinear": lambda c: _ev_resize(c, 1), "upsample2x": _ev_upsample,
         "depth_concat": _ev_depth_concat, "ln_stats": _ev_ln_stats, "ln_finalize": _ev_ln_finalize, "se_scale_add": _ev_se,
         "block_tail": _ev_tail, "spade_apply": _ev_apply, "modulate": _ev_modulate}


def evaluate(family, case):
    with torch.no_grad():
        return _EVAL[family](tuple(case))
