"""Plain reference of the SPADE generator's non-convolution kernels (csrc/spade.hip: resize, upsample2x, depth_concat, ln_stats,
ln_finalize, gap + se_fc + se_scale_add, block_tail, spade_apply and the modulation epilogue), written from the header comments of
include/sln_hip.h and csrc/spade.hip.  CPU tensors in, CPU tensors out, torch and numpy only; no kernel code path is involved.

Every function takes ``dtype``: torch.float64 is the reference, torch.float32 evaluates the SAME formulas and rounds to fp32 where the
kernels store or compute in fp32 - the weights fy, fx, ly, lx of the bilinear forms and the blends, gap and scale of the SE block,
the last three operations of 1 / (sqrt(var) + eps), the elementwise arithmetic.  Reductions (LayerNorm2D sums, the average pool,
the two FCs of the SE block) stay fp64 in both, as in the kernels.  The fp32 result's distance from the fp64 one is the yardstick the
GPU suite holds the kernels to (tests/spade_leaf_cases.py: allowed()).

The nearest index map is the float rule of F.interpolate in BOTH precisions (it is a definition, not an approximation):
src = min(floor(dst * ((float)in / out)), in - 1) evaluated in fp32.
"""
import numpy as np
import torch

D64 = torch.float64
D32 = torch.float32


def _eps(eps, dtype):
    return torch.tensor(eps, dtype=dtype)


# ------------------------------------------------------------------------------------------------ index maps and weights
def nearest_index(n_in, n_out):
    """int64 [n_out]: min(floor(dst * ((float)in / out)), in - 1), every operation in fp32"""
    s = np.float32(n_in) / np.float32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    return torch.from_numpy(np.minimum(np.floor(d * s).astype(np.int64), n_in - 1))


def nearest_index_integer_rule(n_in, n_out):
    """dst * in // out: what the float rule is NOT (they differ at 26 -> 22 and 39 -> 33, among others)"""
    return torch.arange(n_out, dtype=torch.int64) * n_in // n_out


def linear_taps(n_in, n_out, dtype):
    """align_corners=False: f = max((dst + 0.5) * in / out - 0.5, 0); -> (ia, ib int64 [n_out], l [n_out] in dtype), the weight of ib"""
    d = torch.arange(n_out, dtype=dtype)
    s = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    f = ((d + 0.5) * s - 0.5).clamp_min(0)
    ia = f.floor().long().clamp_max(n_in - 1)
    ib = (ia + 1).clamp_max(n_in - 1)
    return ia, ib, f - ia.to(dtype)


def _bilinear(src, Ho, Wo, dtype):
    x = src.to(dtype)
    ya, yb, ly = linear_taps(x.shape[-2], Ho, dtype)
    xa, xb, lx = linear_taps(x.shape[-1], Wo, dtype)
    ly = ly[:, None]
    ra, rb = x[..., ya, :], x[..., yb, :]
    top = (1 - lx) * ra[..., xa] + lx * ra[..., xb]
    bot = (1 - lx) * rb[..., xa] + lx * rb[..., xb]
    return (1 - ly) * top + ly * bot


# ------------------------------------------------------------------------------------------------ resize, upsample
def resize(src, Ho, Wo, mode, dtype=D64):
    """F.interpolate(src, size=(Ho, Wo)) over the last two dimensions: mode 0 nearest (a gather), 1 bilinear, align_corners=False"""
    if mode == 0:
        return src.to(dtype)[..., nearest_index(src.shape[-2], Ho), :][..., nearest_index(src.shape[-1], Wo)]
    return _bilinear(src, Ho, Wo, dtype)


def upsample2x(x, mode, dtype=D64):
    """nn.Upsample(scale_factor=2): mode 0 nearest (source = dst >> 1), 1 bilinear, align_corners=False"""
    H, W = x.shape[-2:]
    if mode == 0:
        return x.to(dtype)[..., torch.arange(2 * H) // 2, :][..., torch.arange(2 * W) // 2]
    return _bilinear(x, 2 * H, 2 * W, dtype)


# ------------------------------------------------------------------------------------------------ 3x3 reflect-padded convolution
def reflect_index(n):
    """source index of padded position 0 .. n + 1 under ReflectionPad2d(1)"""
    i = torch.arange(-1, n + 1).abs()
    return torch.where(i >= n, 2 * n - 2 - i, i)


def conv3x3_reflect(x, w, b, dtype=D64):
    """x [B, Cin, H, W], w [Cout, Cin, 3, 3], b [Cout] or None: bias, then the nine taps in row-major order"""
    B, Cin, H, W = x.shape
    xp = x.to(dtype)[:, :, reflect_index(H), :][:, :, :, reflect_index(W)]
    wd = w.to(dtype)
    out = torch.zeros(B, w.shape[0], H, W, dtype=dtype)
    if b is not None:
        out = out + b.to(dtype).view(1, -1, 1, 1)
    for ky in range(3):
        for kx in range(3):
            out = out + torch.einsum("oc,bchw->bohw", wd[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
    return out


def leaky(x, slope, dtype):
    return torch.where(x > 0, x, x * torch.tensor(slope, dtype=dtype))


def depth_concat(seg, wpd, bpd, nd, dtype=D64):
    """[leaky_0.01(conv3x3_reflect(seg[:, 0:1], 1 -> nd)) | seg[:, 1:]] -> [B, nd + Cs - 1, H, W]; wpd [nd, 9] (or [nd, 1, 3, 3])"""
    d = conv3x3_reflect(seg[:, 0:1], wpd.reshape(nd, 1, 3, 3), bpd, dtype)
    return torch.cat([leaky(d, 0.01, dtype), seg[:, 1:].to(dtype)], 1)


# ------------------------------------------------------------------------------------------------ LayerNorm2D statistics
def _stats_tail(mean, var, eps, dtype):
    """(mean, 1 / (sqrt(var) + eps)) [B, 2]: the sums are fp64, the square root is taken in fp64; its rounding to `dtype`, the
    addition of eps and the reciprocal are the kernel's three fp32 operations"""
    sd = var.clamp_min(0).sqrt().to(dtype)
    return torch.stack([mean.to(dtype), 1.0 / (sd + _eps(eps, dtype))], 1)


def ln_stats(x, eps=1e-5, dtype=D64, rep=1):
    """Two-pass mean and unbiased std over everything but the first dimension -> [B, 2] = (mean, 1 / (std + eps)).
    rep: the statistics of the tensor in which every element of x stands `rep` times (4: its nearest x2 upsampling)"""
    flat = x.to(dtype).double().reshape(x.shape[0], -1)
    n = flat.shape[1]
    mean = flat.sum(1) / n
    var = ((flat - mean[:, None]) ** 2).sum(1) * rep / (n * rep - 1)
    return _stats_tail(mean, var, eps, dtype)


def ln_finalize(s, q, n_acc, rep, eps=1e-5, dtype=D64):
    """The one-pass form from fp64 sums s = sum x, q = sum x^2 over n_acc values, each standing for `rep` elements:
    mean = s / n_acc, var = (rep q - n mean^2) / (n - 1) with n = rep n_acc, clamped at 0"""
    s, q = s.double(), q.double()
    n = float(n_acc) * rep
    mean = s / float(n_acc)
    var = (rep * q - n * mean * mean) / (n - 1.0)
    return _stats_tail(mean, var, eps, dtype)


# ------------------------------------------------------------------------------------------------ squeeze-excite
def se_scale(dx_or_sums, hw, w0, w2, dtype=D64):
    """sigmoid(W2 relu(W0 gap)) [B, C].  dx [B, C, H, W]: gap = the pixel average, stored in `dtype` (the pool kernel writes floats);
    fp64 pixel sums [B, C] (a conv epilogue's): gap = sums / hw, never rounded.  Both FCs and the logistic in fp64; scale in `dtype`."""
    if dx_or_sums.dim() == 4:
        gap = (dx_or_sums.double().sum((2, 3)) / float(hw)).to(dtype).double()
    else:
        gap = dx_or_sums.double() / float(hw)
    hidden = (gap @ w0.double().t()).clamp_min(0)
    return (1.0 / (1.0 + torch.exp(-(hidden @ w2.double().t())))).to(dtype)


def se_scale_add(xs, dx, w0, w2, dtype=D64):
    """x_s + SEBlock2(dx) -> (out [B, C, H, W], scale [B, C])"""
    scale = se_scale(dx, dx.shape[2] * dx.shape[3], w0, w2, dtype)
    return xs.to(dtype) + dx.to(dtype) * scale[:, :, None, None], scale


def block_tail(xs, xs_up, dx, scale, up_mode, dtype=D64, rep=1, eps=1e-5):
    """v = xs + dx * scale[b, c] (xs_up: xs is [B, C, H/2, W/2] and read through nearest x2); out = v (up_mode -1), its nearest (0) or
    bilinear (1) x2 upsampling; stats = LayerNorm2D statistics of what the consumers read: out (rep 1) or its nearest x2 upsampling
    (rep 4).  -> (out, stats [B, 2])"""
    x = upsample2x(xs, 0, dtype) if xs_up else xs.to(dtype)
    v = x + dx.to(dtype) * scale.to(dtype)[:, :, None, None]
    out = v if up_mode < 0 else upsample2x(v, up_mode, dtype)
    return out, ln_stats(out, eps, dtype, rep)


# ------------------------------------------------------------------------------------------------ modulation
def packed_rows(C):
    """rows of gamma and of beta in the packed [32 gamma | 32 beta] layout: row(c) = 64 (c / 32) + c % 32, beta 32 rows further"""
    c = torch.arange(C)
    rg = 64 * (c // 32) + c % 32
    return rg, rg + 32


def _modulate(x, x_up, gamma, beta, stats, act, slope, dtype):
    xv = upsample2x(x, 0, dtype) if x_up else x.to(dtype)
    st = stats.to(dtype)
    v = (xv - st[:, 0].view(-1, 1, 1, 1)) * st[:, 1].view(-1, 1, 1, 1)
    v = v * (1 + gamma) + beta
    return leaky(v, slope, dtype) if act == 2 else v


def spade_apply(x, x_up, gb, stats, C, act, slope, dtype=D64):
    """out[b, c] = ((x[b, c] - mean_b) * inv_b) * (1 + gamma[c]) + beta[c] [-> LeakyReLU(slope), act 2] with gamma / beta the rows
    packed_rows(C) of gb [rows_pad, H, W], shared by the batch; x_up: x is [B, C, H/2, W/2], read through nearest x2"""
    rg, rb = packed_rows(C)
    g = gb.to(dtype)
    return _modulate(x, x_up, g[rg][None], g[rb][None], stats, act, slope, dtype)


def modulate(actv, w_gamma, b_gamma, w_beta, b_beta, xin, xin_up, stats, act, slope=0.2, dtype=D64):
    """SPADE4's tail: LayerNorm2D(xin) * (1 + gamma) + beta [-> LeakyReLU(slope)] with gamma, beta = conv3x3_reflect(actv)"""
    gamma = conv3x3_reflect(actv, w_gamma, b_gamma, dtype)
    beta = conv3x3_reflect(actv, w_beta, b_beta, dtype)
    return _modulate(xin, xin_up, gamma, beta, stats, act, slope, dtype)
