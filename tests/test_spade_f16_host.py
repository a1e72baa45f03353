"""CPU tests of the half-precision conv modes of SPADEGenerator4: the fp16 hi / lo weight packing (host/SPADE_related.py
split_f16 / unpack_f16), the conv_precision switch, and the emulated error budget (tools/spade_half_budget.py)."""
import importlib.util
import os

import pytest
import torch

from conftest import ROOT, load_golden, pkg

from oracle import spade_ref                       # noqa: E402
from oracle.gen_golden_spade import CASES          # noqa: E402


def _budget():
    spec = importlib.util.spec_from_file_location("spade_half_budget", os.path.join(ROOT, "tools", "spade_half_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_split_f16_is_within_its_bound_and_exact_for_fp16_values():
    S = pkg("host.SPADE_related")
    g = torch.Generator().manual_seed(0)
    w = torch.randn(9, 56, 128, generator=g) * torch.logspace(-6, 1.5, 128)          # magnitudes from 1e-6 to 30
    hi, lo = S.split_f16(w)
    assert hi.dtype == lo.dtype == torch.float16 and hi.shape == (4, 9, 128, 16)
    back = S.unpack_f16(hi, lo, 56)
    bound = torch.maximum(w.double().abs() * 2.0 ** -22, torch.full_like(back, 2.0 ** -25))
    assert bool(((back - w.double()).abs() <= bound).all()), float(((back - w.double()).abs() / bound).max())
    exact = w.half().float()
    hi2, lo2 = S.split_f16(exact)
    assert bool((lo2 == 0).all())
    assert torch.equal(S.unpack_f16(hi2, None, 56), exact.double())
    assert bool((hi[:, :, :, :][3, :, :, 8:] == 0).all())                           # channels 56..63: zero padding


def test_packed_layout_round_trips_and_matches_the_kernel_order():
    S = pkg("host.SPADE_related")
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(40, 24, 3, 3, generator=g) * 8).half().float()                # fp16-exact: the round trip is exact
    wp, rp = S._pack(w)
    hi, lo = S.split_f16(wp)
    assert torch.equal(S.unpack_f16(hi, lo, 24), wp.double())
    # element [chunk, tap, row, k] is w[row, 16 chunk + k, tap // 3, tap % 3]
    for (c, t, r, k) in [(0, 0, 0, 0), (1, 4, 39, 7), (0, 8, 17, 15), (1, 2, 5, 3)]:
        assert float(hi[c, t, r, k]) == float(w[r, 16 * c + k, t // 3, t % 3])
    assert float(hi[1, 0, 0, 8].abs()) == 0.0 and float(hi[0, 0, 40, 0].abs()) == 0.0      # channel / row padding
    with pytest.raises(ValueError):
        S.split_f16(torch.zeros(1, 8, 64))


def test_invalid_conv_precision_raises_and_the_packs_follow_the_mode():
    S = pkg("host.SPADE_related")
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    G = S.SPADEGenerator4(cfg.semantic_nc, cfg.target_nc, cfg.nz, cfg.ngf, 'spectralspadelayer3x3', cfg.crop_size, 'normal')
    G.load_state_dict(spade_ref.init_state(cfg, seed=7))
    assert G.conv_precision == "fp32" and S.SPADEGenerator4.conv_precision == "fp32"
    P = G._pack_all()
    assert P["up_3"]["conv_0_h"] is None and P["up_3"]["norm_0"]["wgb_h"] is None
    G.conv_precision = "f16x3"
    P3 = G._pack_all()
    assert P3 is not P and P3["up_3"]["conv_0_h"][1] is not None
    G.conv_precision = "f16"
    P1 = G._pack_all()
    assert P1 is not P3
    assert P1["up_3"]["norm_1"]["wsh_h"][1] is None and P1["up_3"]["conv_1_h"][1] is None
    for name, key in (("head_0", "conv_1_h"), ("up_1", "conv_0_h")):           # the same hi in both half modes, lo in f16x3 only
        assert torch.equal(P1[name][key][0], P3[name][key][0])
        hi, lo = S.split_f16(P3[name][key[:-2]][0])
        assert torch.equal(P3[name][key][0], hi) and torch.equal(P3[name][key][1], lo)
    for bad in ("bf16", "FP32", None, "f16x2"):
        G.conv_precision = bad
        with pytest.raises(ValueError):
            G._pack_all()
        seg, z = spade_ref.synth_input(cfg, 1, seed=3)
        with pytest.raises(ValueError):
            G(seg, z)


def test_emulated_three_product_budget_stays_within_twice_fp32s():
    """The CPU emulation of the modes (tools/spade_half_budget.py) at spade_small: the three-product rounding stays within 2x the
    fp32 rounding's distance from the reference's own image (tests/golden/spade_small.npz); the one-product rounding does not."""
    B = _budget()
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    sd = spade_ref.init_state(cfg, seed=7)
    seg, z = spade_ref.synth_input(cfg, CASES["spade_small"][1], seed=3)
    ref = torch.from_numpy(load_golden("spade_small")["out"]).double()
    err = {m: float((B.emulate(sd, cfg, seg, z, m) - ref).abs().max()) for m in B.MODES}
    assert err["f16x3"] <= 2 * err["fp32"], err
    assert err["f16"] > 10 * err["fp32"], err
