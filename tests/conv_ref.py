"""fp64 yardstick of the SPADE generator's convolutions (csrc/spade.hip conv_mfma_kernel / conv_glds_kernel / conv_f16_kernel),
written from the definitions; torch only, the library is never imported here.  tests/test_conv_ref_host.py holds these functions
to F.conv2d in double and to a six-deep Python loop.

    out[b, o, y, x] = bias[o] + sum_{c, ky, kx} w[o, c, ky, kx] * xpad[b, c, y + ky, x + kx]          (3x3, ReflectionPad2d(1))
    out[b, o, y, x] = bias[o] + sum_c w[o, c, 0, 0] * x[b, c, y, x]                                   (1x1)
"""
import torch

D64 = torch.float64
F16_MAX = 65504.0
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def reflect_index(n):
    """Source index of every position of a length-n axis padded by one on both sides: -1 -> 1, n -> n - 2."""
    if n < 2:
        raise ValueError("reflection by one needs two samples")
    return torch.tensor([1] + list(range(n)) + [n - 2], dtype=torch.long)


def reflect_pad1(x):
    return x.index_select(2, reflect_index(x.shape[2])).index_select(3, reflect_index(x.shape[3]))


def conv(x, w, bias=None):
    """x [B, Cin, H, W], w [Cout, Cin, k, k] (k = 1 or 3), bias [Cout] or None -> [B, Cout, H, W], everything in fp64."""
    x, w = x.to(D64), w.to(D64)
    B, _, H, W = x.shape
    k = w.shape[2]
    if k not in (1, 3) or w.shape[3] != k:
        raise ValueError("1x1 or 3x3")
    xp = reflect_pad1(x) if k == 3 else x
    out = torch.zeros(B, w.shape[0], H, W, dtype=D64)
    for ky in range(k):
        for kx in range(k):
            out += torch.einsum("oc,bchw->bohw", w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
    if bias is not None:
        out += bias.to(D64).view(1, -1, 1, 1)
    return out


def conv_abs(x, w, bias=None):
    """sum of the magnitudes of every term of conv(): what the rounding bounds and the exactness conditions are stated in."""
    return conv(x.to(D64).abs(), w.to(D64).abs(), None if bias is None else bias.to(D64).abs())


def activate(v, act, slope):
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, v * slope)
    raise ValueError(act)


def upsample_nearest2(x):
    """nn.Upsample(scale_factor=2, mode='nearest'): out[.., y, x] = in[.., y // 2, x // 2]."""
    H, W = x.shape[2], x.shape[3]
    iy = torch.arange(2 * H) // 2
    ix = torch.arange(2 * W) // 2
    return x.index_select(2, iy).index_select(3, ix)


def modulate(gamma, beta, xin, xin_up, stats, act, slope):
    """LN(xin) * (1 + gamma) + beta [-> activation]; stats [B, 2] = (mean, 1 / (std + eps)); xin_up: xin is [B, C, H / 2, W / 2]."""
    xin = xin.to(D64)
    if xin_up:
        xin = upsample_nearest2(xin)
    st = stats.to(D64)
    norm = (xin - st[:, 0].view(-1, 1, 1, 1)) * st[:, 1].view(-1, 1, 1, 1)
    return activate(norm * (1.0 + gamma) + beta, act, slope)


def sums(y):
    """-> (ln [B, 2] = sum y, sum y^2 of each sample; gap [B, rows] = sum over pixels), of the fp64 tensor y."""
    y = y.to(D64)
    return torch.stack([y.sum((1, 2, 3)), (y * y).sum((1, 2, 3))], 1), y.sum((2, 3))


# ------------------------------------------------------------------------------------------------ the half modes
def f16_round(v):
    """fp16(clamp(v)) as fp64: what an operand of the one-product mode is."""
    return v.to(D64).clamp(-F16_MAX, F16_MAX).to(torch.float32).to(torch.float16).to(D64)


def f16_split(v):
    """-> (hi, lo) of the three-product mode, as fp64: hi = fp16(clamp(v)), lo = fp16(clamp(v) - hi) (v is fp32 data: the
    difference is exact in fp32, so one rounding, to fp16)."""
    c = v.to(D64).clamp(-F16_MAX, F16_MAX)
    hi = c.to(torch.float32).to(torch.float16).to(D64)
    lo = (c - hi).to(torch.float32).to(torch.float16).to(D64)
    return hi, lo


def conv_one_product(x, w_hi, bias=None):
    """sum w_hi * x_hi: w_hi is the weight pack's own hi part [Cout, Cin, 3, 3]."""
    return conv(f16_round(x), w_hi, bias)


def conv_three_products(x, w_hi, w_lo, bias=None):
    """sum (w_hi x_hi + w_hi x_lo + w_lo x_hi), w_hi / w_lo the pack's own parts; the dropped w_lo x_lo is not in it."""
    xh, xl = f16_split(x)
    return conv(xh, w_hi, bias) + conv(xl, w_hi) + conv(xh, w_lo)


def conv_three_products_abs(x, w_hi, w_lo, bias=None):
    xh, xl = f16_split(x)
    return conv_abs(xh, w_hi, bias) + conv_abs(xl, w_hi) + conv_abs(xh, w_lo)


def gamma_bound(n, u=2.0 ** -24):
    """gamma_n = n u / (1 - n u): the relative bound of n roundings to nearest in any order (Higham, Accuracy and Stability, 3.1)."""
    return n * u / (1.0 - n * u)
