"""The fp64 yardstick of the convolution family tests (tests/conv_ref.py) against torch's own double convolution and against a
six-deep Python loop, and the properties of the seeded operands (tests/conv_cases.py) that the exact groups rest on.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as K
import conv_ref as R

D64 = torch.float64


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=D64)


@pytest.mark.parametrize("B,Cin,H,W,Cout,k", [(2, 5, 9, 18, 7, 3), (1, 3, 2, 2, 4, 3), (3, 4, 7, 5, 6, 1), (1, 17, 17, 3, 5, 3)])
def test_conv_matches_torch_double(B, Cin, H, W, Cout, k):
    x, w, b = _rand((B, Cin, H, W), 1), _rand((Cout, Cin, k, k), 2), _rand((Cout,), 3)
    ref = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect") if k == 3 else x, w, b)
    got = R.conv(x, w, b)
    assert got.dtype == D64 and float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    assert torch.equal(R.reflect_pad1(x), F.pad(x, (1, 1, 1, 1), mode="reflect"))
    assert float((R.conv_abs(x, w, b) - F.conv2d(F.pad(x.abs(), (1, 1, 1, 1), mode="reflect") if k == 3 else x.abs(), w.abs(), b.abs())).abs().max()) <= 1e-12


def test_conv_matches_a_six_deep_loop():
    B, Cin, H, W, Cout = 2, 3, 3, 2, 2
    x, w, b = _rand((B, Cin, H, W), 4), _rand((Cout, Cin, 3, 3), 5), _rand((Cout,), 6)

    def refl(i, n):
        i = -i if i < 0 else i
        return 2 * n - 2 - i if i >= n else i
    ref = torch.zeros(B, Cout, H, W, dtype=D64)
    for bi in range(B):
        for o in range(Cout):
            for y in range(H):
                for xx in range(W):
                    s = float(b[o])
                    for c in range(Cin):
                        for t in range(9):
                            s += float(w[o, c, t // 3, t % 3]) * float(x[bi, c, refl(y + t // 3 - 1, H), refl(xx + t % 3 - 1, W)])
                    ref[bi, o, y, xx] = s
    assert float((R.conv(x, w, b) - ref).abs().max()) <= 1e-13
    # the 1x1 form
    w1 = _rand((Cout, Cin, 1, 1), 7)
    ref1 = torch.stack([torch.stack([sum(w1[o, c, 0, 0] * x[bi, c] for c in range(Cin)) + b[o] for o in range(Cout)]) for bi in range(B)])
    assert float((R.conv(x, w1, b) - ref1).abs().max()) <= 1e-13


@pytest.mark.parametrize("xin_up", [0, 1])
def test_modulation_activation_and_sums_match_torch(xin_up):
    B, C, H, W = 2, 5, 4, 6
    gamma, beta = _rand((B, C, H, W), 8), _rand((B, C, H, W), 9)
    xin = _rand((B, C, H // 2, W // 2) if xin_up else (B, C, H, W), 10)
    stats = torch.tensor([[0.25, 1.5], [-1.0, 0.75]], dtype=D64)
    xf = F.interpolate(xin, scale_factor=2, mode="nearest") if xin_up else xin
    norm = (xf - stats[:, 0].view(B, 1, 1, 1)) * stats[:, 1].view(B, 1, 1, 1)
    ref = F.leaky_relu(norm * (1 + gamma) + beta, 0.2)
    assert float((R.modulate(gamma, beta, xin, xin_up, stats, R.ACT_LEAKY, 0.2) - ref).abs().max()) <= 1e-14
    assert torch.equal(R.modulate(gamma, beta, xin, xin_up, stats, R.ACT_NONE, 0.2), norm * (1 + gamma) + beta)
    assert torch.equal(R.activate(gamma, R.ACT_RELU, 0.0), F.relu(gamma))
    ln, gap = R.sums(ref)
    assert torch.allclose(ln[:, 0], ref.flatten(1).sum(1), rtol=1e-14) and torch.allclose(ln[:, 1], (ref ** 2).flatten(1).sum(1), rtol=1e-14)
    assert gap.shape == (B, C) and torch.allclose(gap, ref.sum((2, 3)), rtol=1e-14)


def test_half_mode_answers_are_built_from_the_fp16_parts():
    x = torch.tensor([1.0 + 2.0 ** -12, -1.0 + 2.0 ** -12, 2.0 ** -12, 1.0e5, -7.0e4, 0.1, 3.0e-6, 0.0], dtype=D64).view(1, 8, 1, 1).expand(1, 8, 2, 2).contiguous()
    hi, lo = R.f16_split(x)
    assert hi.flatten()[0::4].tolist()[:5] == [1.0, -1.0, 2.0 ** -12, 65504.0, -65504.0]
    assert lo.flatten()[0::4].tolist()[:5] == [2.0 ** -12, 2.0 ** -12, 0.0, 0.0, 0.0]
    assert torch.equal(R.f16_round(x), hi)
    v = x.clamp(-65504, 65504)
    assert float((hi + lo - v).abs().max()) <= 2.0 ** -22 * 0.1 + 2.0 ** -25                 # the split's representation error
    w = _rand((3, 8, 3, 3), 11).float().double()
    w_hi, w_lo = R.f16_split(w)
    b = _rand((3,), 12)
    assert torch.equal(R.conv_one_product(x, w_hi, b), R.conv(hi, w_hi, b))
    three = R.conv_three_products(x, w_hi, w_lo, b)
    full = R.conv(hi + lo, w_hi + w_lo, b)
    assert float((three - (full - R.conv(lo, w_lo))).abs().max()) <= 1e-9 * float(full.abs().max())
    assert R.gamma_bound(100) == pytest.approx(100 * 2.0 ** -24, rel=1e-5) and R.gamma_bound(100) > 100 * 2.0 ** -24


def test_case_names_are_unique_and_the_named_groups_exist():
    assert len(K.CASES) == len(K.BY_NAME) == 28 + 28
    for name in K.GAUSSIAN:
        assert K.BY_NAME[name].entry == K.CONV
    for name in K.PADDING:
        c = K.BY_NAME[name]
        assert (2 * c.rows if c.entry == K.MOD else c.rows) < c.rows_pad
    for c in K.CASES:
        assert c.rows_pad % 64 == 0 and c.B * max(c.Cin, c.rows) * c.H * c.W < 4_000_000, c.name          # the largest tensor


@pytest.mark.parametrize("name", ["staged-3x3-64", "dma-3x3-split-128", "f16-split-64-t3", "f16-mod-up-128-t3", "dma-1x1-split-64"])
def test_operand_generators_keep_their_promises(name):
    c = K.BY_NAME[name]
    d = K.integer_operands(c)
    w = d["w"] if c.entry == K.CONV else d["wg"]
    assert d["x"].abs().max() <= 2 and w.abs().max() <= 2 and torch.equal(d["x"], d["x"].round()) and torch.equal(w, w.round())
    assert torch.equal(K.integer_operands(c)["x"], d["x"])                                               # seeded
    if c.ksize == 3:
        for lo_in_x in (True, False):
            d = K.lattice_operands(c, lo_in_x)
            w = d["w"] if c.entry == K.CONV else d["wg"]
            for t, has_lo in ((d["x"], lo_in_x), (w, not lo_in_x)):
                hi, lo = R.f16_split(t)
                assert set(hi.unique().tolist()) <= {-1.0, 0.0, 1.0}
                assert set(lo.unique().tolist()) <= ({-K.LATTICE_LO, 0.0, K.LATTICE_LO} if has_lo else {0.0})
                assert torch.equal(hi + lo, t)
                if has_lo:
                    assert torch.equal(lo != 0, hi != 0)
    g = K.gaussian_operands(c)
    assert all(torch.equal(v, v.float().double()) for v in g.values())
    if c.terms:
        assert g["x"].abs().max() > 65504 and (g["x"].abs() < 2.0 ** -14).any()
