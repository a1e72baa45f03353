"""Case table and seeded operands of the SPADE convolution family tests, shared by tests/test_conv_route_host.py (the routes the
table claims against sln_debug_conv_route) and tests/test_conv_family_gpu.py (every case through the public entry points).  torch
only; the library is never imported here.

A case names the kernel it is there for.  Route = (kernel, bmc, tile_h, gk, blk, terms, shares) as SlnDbgConvRoute reports it:
kernel "staged" (conv_mfma_kernel), "dma" (conv_glds_kernel) or "f16" (conv_f16_kernel); bmc packed rows per workgroup; tile_h x 16
pixels per workgroup; gk input channels per chunk; blk chunks per accumulation block; shares > 1: the input-channel split.

`route` holds with no switch set (force 0).  With SLN_CONV_DMA (force 2) a case takes `route_dma` where one is given, with
SLN_CONV_STAGED (force 1) every fp32 case takes the staged kernel (route_for); the half modes know no switch.
"""
import zlib
from collections import namedtuple

import torch

STAGED, DMA, F16 = "staged", "dma", "f16"
KERNEL_IDS = {0: STAGED, 1: DMA, 2: F16}
CONV, MOD = "conv", "mod"          # sln_spade_conv_sums[_f16] (bias + activation) / sln_spade_modulate_up[_f16]
BLOCK_CIN = 512                     # 3x3 bias/activation convolutions of at least this many input channels accumulate in blocks

Case = namedtuple("Case", "name entry terms B Cin H W rows rows_pad ksize xin_up route route_dma")


def _rows_pad(entry, rows):
    return 64 * ((rows + 31) // 32) if entry == MOD else (rows + 63) // 64 * 64


def _c(name, entry, terms, B, Cin, H, W, rows, route, ksize=3, xin_up=0, rows_pad=None, route_dma=None):
    return Case(name, entry, terms, B, Cin, H, W, rows, rows_pad or _rows_pad(entry, rows), ksize, xin_up, route, route_dma)


# ------------------------------------------------------------------------------------------------ fp32
FP32_CASES = [
    # conv_mfma_kernel<BMC, KS, EPI, BLK>: 8
    _c("staged-3x3-64", CONV, 0, 2, 5, 9, 18, 33, (STAGED, 64, 8, 8, 0, 0, 1)),
    _c("staged-3x3-128", CONV, 0, 2, 41, 10, 17, 130, (STAGED, 128, 8, 8, 0, 0, 1), rows_pad=256),
    _c("staged-1x1-64", CONV, 0, 3, 3, 7, 5, 130, (STAGED, 64, 8, 8, 0, 0, 1), ksize=1),
    _c("staged-1x1-128", CONV, 0, 2, 9, 8, 16, 65, (STAGED, 128, 8, 8, 0, 0, 1), ksize=1),
    _c("staged-blocked-64", CONV, 0, 1, 516, 5, 6, 33, (STAGED, 64, 8, 8, 2, 0, 1)),
    _c("staged-blocked-128", CONV, 0, 1, 516, 5, 6, 100, (STAGED, 128, 8, 8, 2, 0, 1)),
    _c("staged-mod-64", MOD, 0, 2, 12, 9, 17, 8, (STAGED, 64, 8, 8, 0, 0, 1)),
    _c("staged-mod-64-up", MOD, 0, 2, 12, 10, 18, 70, (STAGED, 64, 8, 8, 0, 0, 1), xin_up=1),
    _c("staged-mod-128", MOD, 0, 2, 12, 9, 17, 33, (STAGED, 128, 8, 8, 0, 0, 1)),
    # conv_glds_kernel<BMC, KS, EPI, 8, 4, BLK>: 8 x 16 pixels
    _c("dma-blocked-split-64", CONV, 0, 1, 512, 9, 17, 33, (DMA, 64, 8, 4, 4, 0, 16)),
    _c("dma-blocked-split-128", CONV, 0, 1, 520, 9, 17, 100, (DMA, 128, 8, 4, 4, 0, 16)),          # shares of 12 chunks: 11 work, 5 idle
    _c("dma-blocked-64", CONV, 0, 192, 512, 3, 5, 33, (DMA, 64, 8, 4, 4, 0, 1)),
    _c("dma-blocked-128", CONV, 0, 192, 512, 3, 5, 100, (DMA, 128, 8, 4, 4, 0, 1)),
    _c("dma-3x3-split-64", CONV, 0, 1, 68, 9, 17, 33, (DMA, 64, 8, 4, 0, 0, 2)),                     # 9 and 8 chunks
    _c("dma-3x3-split-128", CONV, 0, 2, 64, 2, 2, 200, (DMA, 128, 8, 4, 0, 0, 2)),                   # plane 4: the one-wavefront finish
    _c("dma-1x1-split-64", CONV, 0, 1, 100, 7, 20, 130, (DMA, 64, 8, 4, 0, 0, 3), ksize=1),
    _c("dma-1x1-split-128", CONV, 0, 2, 132, 9, 9, 65, (DMA, 128, 8, 4, 0, 0, 4), ksize=1),         # 9, 9, 9, 6 chunks
    _c("dma-mod-64", MOD, 0, 2, 16, 9, 17, 8, (DMA, 64, 8, 4, 0, 0, 1)),
    _c("dma-mod-128-up", MOD, 0, 3, 8, 2, 2, 33, (DMA, 128, 8, 4, 0, 0, 1), xin_up=1),
    # conv_glds_kernel<BMC, 3, EPI, 16, GK, BLK>: 16 x 16 pixels
    _c("tall-blocked-64", CONV, 0, 64, 512, 17, 3, 200, (DMA, 64, 16, 8, 2, 0, 1)),
    _c("tall-3x3-64", CONV, 0, 43, 24, 17, 18, 130, (DMA, 64, 16, 8, 0, 0, 1)),
    _c("tall-3x3-128", CONV, 0, 64, 24, 17, 18, 200, (DMA, 128, 16, 4, 0, 0, 1)),
    _c("tall-mod-64-up", MOD, 0, 43, 24, 18, 20, 70, (DMA, 64, 16, 8, 0, 0, 1), xin_up=1),
    _c("tall-mod-128", MOD, 0, 128, 24, 18, 20, 33, (DMA, 128, 16, 4, 0, 0, 1)),
    # staged by default, the unsplit 8 x 16 DMA kernel under SLN_CONV_DMA
    _c("switch-3x3-64", CONV, 0, 2, 16, 9, 18, 33, (STAGED, 64, 8, 8, 0, 0, 1), route_dma=(DMA, 64, 8, 4, 0, 0, 1)),
    _c("switch-3x3-128", CONV, 0, 2, 8, 10, 17, 130, (STAGED, 128, 8, 8, 0, 0, 1), rows_pad=256, route_dma=(DMA, 128, 8, 4, 0, 0, 1)),
    _c("switch-1x1-64", CONV, 0, 3, 8, 7, 5, 130, (STAGED, 64, 8, 8, 0, 0, 1), ksize=1, route_dma=(DMA, 64, 8, 4, 0, 0, 1)),
    _c("switch-1x1-128", CONV, 0, 2, 16, 8, 16, 65, (STAGED, 128, 8, 8, 0, 0, 1), ksize=1, route_dma=(DMA, 128, 8, 4, 0, 0, 1)),
]


# ------------------------------------------------------------------------------------------------ half
def _half(name, entry, B, Cin, H, W, rows, tile_h, blk, shares, xin_up=0, tile_h_3=None):
    bmc = 128 if _rows_pad(entry, rows) % 128 == 0 else 64
    return [_c("%s-%d-t%d" % (name, bmc, t), entry, t, B, Cin, H, W, rows,
               (F16, bmc, tile_h_3 if (t == 3 and tile_h_3) else tile_h, 16, blk, t, shares), xin_up=xin_up) for t in (1, 3)]


HALF_CASES = sum([
    _half("f16-3x3", CONV, 2, 17, 9, 18, 33, 8, 0, 1) + _half("f16-3x3", CONV, 2, 17, 9, 18, 100, 8, 0, 1),
    # 9 chunks, the last half empty; 4 shares of 3, 3, 3, 0 chunks become 3
    _half("f16-split", CONV, 1, 136, 9, 17, 33, 8, 0, 3) + _half("f16-split", CONV, 1, 136, 9, 17, 100, 8, 0, 3),
    _half("f16-blocked-split", CONV, 1, 520, 9, 17, 33, 8, 1, 11) + _half("f16-blocked-split", CONV, 1, 520, 9, 17, 100, 8, 1, 11),
    _half("f16-blocked", CONV, 192, 512, 3, 5, 33, 8, 1, 1) + _half("f16-blocked", CONV, 192, 512, 3, 5, 100, 8, 1, 1),
    # (no 16 x 16 x 128-row three-product kernel: 8 x 16 there)
    _half("f16-tall", CONV, 43, 24, 17, 18, 130, 16, 0, 1) + _half("f16-tall", CONV, 64, 24, 17, 18, 200, 16, 0, 1, tile_h_3=8),
    _half("f16-mod", MOD, 2, 16, 9, 17, 8, 8, 0, 1) + _half("f16-mod-up", MOD, 3, 8, 2, 2, 33, 8, 0, 1, xin_up=1),
    _half("f16-tall-mod-up", MOD, 43, 24, 18, 20, 70, 16, 0, 1, xin_up=1) + _half("f16-tall-mod", MOD, 128, 24, 18, 20, 33, 16, 0, 1, tile_h_3=8),
], [])

CASES = FP32_CASES + HALF_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def route_for(case, force):
    """The route the table claims under force 0 (no switch), 1 (SLN_CONV_STAGED) or 2 (SLN_CONV_DMA)."""
    if case.terms != 0 or force == 0:
        return case.route
    if force == 1:
        blocked = case.entry == CONV and case.ksize == 3 and case.Cin >= BLOCK_CIN
        return (STAGED, 128 if case.rows_pad % 128 == 0 else 64, 8, 8, 2 if blocked else 0, 0, 1)
    if force == 2:
        return case.route_dma or case.route
    raise ValueError(force)


def kernel_of(case, route):
    """The instantiation a route stands for, with the split form told apart: (kernel, bmc, ksize, epi, tile_h, gk, blk, terms, split)."""
    return (route[0], route[1], case.ksize, 1 if case.entry == MOD else 0, route[2], route[3], route[4], route[5], route[6] > 1)


# ------------------------------------------------------------------------------------------------ operands
SLOPE = 0.25                 # LeakyReLU slope of the exact groups: a power of two
MOD_MEAN, MOD_INV = 1.0, 0.5


def _gen(kind, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((kind, case.name)).encode()))


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _weights(case, draw):
    """-> dict: conv: w [Cout, Cin, k, k], b [Cout];  mod: wg, wb [C, Cin, 3, 3], bg, bb [C], xin, stats."""
    k, n = case.ksize, case.rows
    if case.entry == CONV:
        return dict(w=draw("w", (n, case.Cin, k, k)), b=draw("b", (n,)))
    hx, wx = (case.H // 2, case.W // 2) if case.xin_up else (case.H, case.W)
    return dict(wg=draw("w", (n, case.Cin, 3, 3)), wb=draw("w", (n, case.Cin, 3, 3)), bg=draw("b", (n,)), bb=draw("b", (n,)),
                xin=draw("xin", (case.B, n, hx, wx)),
                stats=torch.tensor([[MOD_MEAN, MOD_INV]] * case.B, dtype=torch.float64))


def integer_operands(case):
    """x, w in {-2 .. 2}, bias in {-8 .. 8}, xin in {-4 .. 4}, stats (1, 0.5): every product, partial sum, share and epilogue value is
    an exactly representable number in fp32 (operands: in fp16 too) whatever the order, as long as sum |terms| < 2^24."""
    g = _gen("int", case)
    rng = dict(x=2, w=2, b=8, xin=4)
    d = _weights(case, lambda what, shape: _randint(g, -rng[what], rng[what], shape))
    d["x"] = _randint(g, -2, 2, (case.B, case.Cin, case.H, case.W))
    return d


LATTICE_LO = 2.0 ** -12
LATTICE_TERMS = 16.0         # expected non-zero products per output (sigma 4): sum |terms| stays far below 2^6


def lattice_operands(case, lo_in_x):
    """Operands h + l with h in {-1, 0, 1} and l in {-2^-12, +2^-12} where h != 0 (l = 0 where h = 0, or in the operand that carries
    no lo at all): fp16(h + l) = h and lo = l exactly.  The density of non-zeros keeps sum |terms| < 2^6 per output.  lo sits in x
    (lo_in_x) or in the weights, never in both: no sum leaves the 2^-12 grid."""
    g = _gen("lattice", case)
    p = min(1.0, (LATTICE_TERMS / (case.ksize ** 2 * case.Cin)) ** 0.5)

    def tern(shape, with_lo):
        h = (torch.rand(shape, generator=g) < p).double() * (2.0 * torch.randint(0, 2, shape, generator=g).double() - 1.0)
        if with_lo:
            h = h + h.abs() * LATTICE_LO * (2.0 * torch.randint(0, 2, shape, generator=g).double() - 1.0)
        return h

    def draw(what, shape):
        if what == "w":
            return tern(shape, not lo_in_x)
        if what == "b":
            return _randint(g, -2, 2, shape)
        return _randint(g, -4, 4, shape)              # xin
    d = _weights(case, draw)
    d["x"] = tern((case.B, case.Cin, case.H, case.W), lo_in_x)
    return d


def gaussian_operands(case):
    """Ordinary data: x ~ N(0.3, 1), w ~ N(0, 1 / K), b ~ N(0, 1).  The half modes get, in a few places of x, magnitudes past the
    fp16 range (clamped to +-65504 by the kernel) and values around 1e-5 and 1e-7 (lo below fp16's normal range, 2^-14)."""
    g = _gen("gauss", case)
    K = case.ksize ** 2 * case.Cin
    d = _weights(case, lambda what, shape: torch.randn(shape, generator=g).float().double() * (K ** -0.5 if what == "w" else 1.0))
    x = (torch.randn(case.B, case.Cin, case.H, case.W, generator=g) + 0.3).float()
    if case.terms:
        flat = x.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:24]
        flat[idx[:4]] = torch.tensor([1.0e5, -1.0e5, 70000.0, -65520.0])
        flat[idx[4:14]] *= 1.0e-5
        flat[idx[14:24]] *= 1.0e-7
    d["x"] = x.double()
    return {k: v.float().double() for k, v in d.items()}


# the Gaussian group: one bias/activation case per kernel family and accumulation form
GAUSSIAN = ["staged-3x3-128", "staged-1x1-64", "staged-blocked-128", "dma-3x3-split-64", "dma-1x1-split-128", "dma-blocked-split-128",
            "dma-blocked-64", "tall-3x3-64", "tall-blocked-64",
            "f16-3x3-64-t1", "f16-3x3-128-t3", "f16-split-128-t1", "f16-split-64-t3", "f16-blocked-split-64-t1",
            "f16-blocked-split-128-t3", "f16-blocked-128-t1", "f16-blocked-64-t3", "f16-tall-64-t1", "f16-tall-64-t3"]
# padding that must not leak: a bias/activation and a modulation case per kernel family, rows < rows_pad in all of them
PADDING = ["staged-3x3-128", "staged-mod-128", "dma-blocked-split-128", "dma-mod-128-up", "tall-3x3-64",
           "f16-split-128-t1", "f16-split-128-t3", "f16-mod-up-128-t1", "f16-mod-up-128-t3", "f16-tall-mod-up-64-t3"]
