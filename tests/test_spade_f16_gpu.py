"""GPU tests of the opt-in fp16-MFMA precision modes of the SPADE generator's 3x3 convolutions (run with -m gpu):
conv_f16_kernel through sln_spade_conv_sums_f16 / sln_spade_modulate_up_f16 against fp64 known answers, and
SPADEGenerator4.conv_precision = "f16x3" / "f16" end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden, pkg
from parity import assert_close

pytestmark = pytest.mark.gpu

from oracle import spade_ref                       # noqa: E402
from oracle.gen_golden_spade import CASES          # noqa: E402


def _budget():
    spec = importlib.util.spec_from_file_location("spade_half_budget", os.path.join(ROOT, "tools", "spade_half_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _f16(t):
    return t.clamp(-65504.0, 65504.0).half().double()


def _ref_conv(x, w, b):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)


def _gen(cfg, seed):
    S = pkg("host.SPADE_related")
    G = S.SPADEGenerator4(cfg.semantic_nc, cfg.target_nc, cfg.nz, cfg.ngf, 'spectralspadelayer3x3', cfg.crop_size, 'normal')
    G.load_state_dict(spade_ref.init_state(cfg, seed=seed))
    return G.cuda().eval()


# (B, Cin, Cout, H, W): input-channel split with the sums (Cin 56: padded chunk), 16 x 16-pixel tiles, blocked + split, plain 8 x 16
CONV_CASES = [(3, 56, 100, 20, 24), (8, 32, 128, 128, 128), (2, 512, 64, 16, 16), (16, 48, 64, 64, 64)]


@pytest.mark.parametrize("B,Cin,Cout,H,W", CONV_CASES)
def test_conv_f16_known_answers_and_sums(B, Cin, Cout, H, W):
    """One product: fp64 conv of the fp16-ROUNDED operands (fp16 products are exact in fp32: only the accumulation differs);
    three products: fp64 conv of the unrounded operands.  Both within 2x the fp32 kernel's own error on the same shape (a kernel
    that does not round, such as the fp32 one, misses the one-product bound by the rounding itself).  The epilogue's LayerNorm and
    pixel sums are those of what it wrote."""
    L = pkg("_lib"); S = pkg("host.SPADE_related")
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    x = torch.randn(B, Cin, H, W, generator=g) + 0.3
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    b = torch.randn(Cout, generator=g)
    xd = x.cuda()
    wp, rp = S._pack(w.cuda())
    bp = torch.zeros(rp, device="cuda"); bp[:Cout] = b.cuda()
    hi, lo = S.split_f16(wp)
    ref = F.leaky_relu(_ref_conv(x.double(), w.double(), b.double()), 0.2)
    w_r = S.unpack_f16(hi, None, Cin).cpu()[:, :, :Cout].permute(2, 1, 0).reshape(Cout, Cin, 3, 3)
    ref_r = F.leaky_relu(_ref_conv(_f16(x), w_r, b.double()), 0.2)
    assert torch.equal(w_r, _f16(w))

    def run(fn, *wargs):
        y = torch.empty(B, Cout, H, W, device="cuda")
        ln = torch.zeros(16 * B, dtype=torch.float64, device="cuda"); gap = torch.zeros(B, Cout, dtype=torch.float64, device="cuda")
        L.check(fn(L.ptr(xd), B, Cin, H, W, *wargs, L.ptr(bp), Cout, rp, 3, 2, 0.2, L.ptr(y), L.ptr(ln), L.ptr(gap), L.current_stream_ptr()), "conv")
        torch.cuda.synchronize()
        yd = y.double().cpu()
        assert_close(ln.view(B, 16)[:, 0].cpu().numpy(), yd.sum((1, 2, 3)).numpy(), "sum", rtol=1e-6, atol=1e-4)
        assert_close(gap.cpu().numpy(), yd.sum((2, 3)).numpy(), "pixel sums", rtol=1e-5, atol=1e-4)
        return yd
    lib = L.lib()
    e32 = float((run(lib.sln_spade_conv_sums, L.ptr(wp)) - ref).abs().max())
    e1 = float((run(lib.sln_spade_conv_sums_f16, L.ptr(hi), None) - ref_r).abs().max())
    y3 = run(lib.sln_spade_conv_sums_f16, L.ptr(hi), L.ptr(lo))
    # the three products of the split operands in fp64: what the kernel computes up to its fp32 accumulation.  The split itself is
    # 2^-22 relative - except that lo is fp16: below 2^-14 it is subnormal, steps of 2^-24 (|w| < 2^-3: the Cin = 512 case, weights
    # ~0.015, is 4x the fp32 kernel's blocked figure from that alone, split_f16's documented bound)
    xs = x.double().clamp(-65504.0, 65504.0)
    xh, xl = _f16(xs), _f16(xs - _f16(xs))
    w_l = S.unpack_f16(lo, None, Cin).cpu()[:, :, :Cout].permute(2, 1, 0).reshape(Cout, Cin, 3, 3)
    ref3 = F.leaky_relu(_ref_conv(xh, w_r, b.double()) + _ref_conv(xl, w_r, None) + _ref_conv(xh, w_l, None), 0.2)
    e3 = float((y3 - ref3).abs().max())
    e_split = float((ref3 - ref).abs().max())
    bound = 2 * e32 + 1e-7
    assert e1 <= bound, ("one product vs fp64 of the fp16-rounded operands", e1, "bound 2 x fp32 kernel", bound)
    assert e3 <= bound, ("three products vs fp64 of the split operands", e3, "bound 2 x fp32 kernel", bound)
    e3u = float((y3 - ref).abs().max())
    assert e3u <= bound + e_split, ("three products vs fp64 of the unrounded operands", e3u, "bound 2 x fp32 kernel + split", bound + e_split)
    assert e_split <= 8 * e32 + 1e-7, ("representation error of the hi / lo split", e_split, e32)
    # the one-product mode really rounds: it is far from the unrounded answer
    assert float((run(lib.sln_spade_conv_sums_f16, L.ptr(hi), None) - ref).abs().max()) > 10 * bound


# (B, Cin, C, H, W, xin_up): 128-row blocks 8 x 16 px, 64-row blocks with the upsampled input, 16 x 16 px with the upsampled input
MOD_CASES = [(2, 128, 64, 32, 32, 0), (4, 128, 32, 24, 40, 1), (8, 32, 32, 128, 128, 1)]


@pytest.mark.parametrize("B,Cin,C,H,W,xin_up", MOD_CASES)
def test_modulate_f16_known_answers(B, Cin, C, H, W, xin_up):
    L = pkg("_lib"); S = pkg("host.SPADE_related")
    g = torch.Generator().manual_seed(C + 3 * H)
    actv = torch.relu(torch.randn(B, Cin, H, W, generator=g))
    hx, wx = (H // 2, W // 2) if xin_up else (H, W)
    xin = torch.randn(B, C, hx, wx, generator=g) * 2 + 0.5
    wg = torch.randn(C, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5; bg = torch.randn(C, generator=g) * 0.1
    wb = torch.randn(C, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5; bb = torch.randn(C, generator=g) * 0.1
    wgb, bgb, rpg = S._pack_gamma_beta(wg.cuda(), bg.cuda(), wb.cuda(), bb.cuda())
    hi, lo = S.split_f16(wgb)
    xu = F.interpolate(xin, scale_factor=2, mode="nearest") if xin_up else xin
    flat = xu.double().reshape(B, -1)
    mean, std = flat.mean(1), flat.std(1)
    stats = torch.stack([mean, 1.0 / (std + 1e-5)], 1).float()
    norm = (xu.double() - stats[:, 0].double().view(B, 1, 1, 1)) * stats[:, 1].double().view(B, 1, 1, 1)

    def ref_of(a, wgr, wbr):
        return F.leaky_relu(norm * (1 + _ref_conv(a, wgr, bg.double())) + _ref_conv(a, wbr, bb.double()), 0.2)
    ref = ref_of(actv.double(), wg.double(), wb.double())
    ref_r = ref_of(_f16(actv), _f16(wg), _f16(wb))
    ad, xd, sd = actv.cuda(), xin.cuda(), stats.cuda()

    def run(fn, *wargs):
        out = torch.empty(B, C, H, W, device="cuda")
        L.check(fn(L.ptr(ad), B, Cin, H, W, *wargs, L.ptr(bgb), C, rpg, L.ptr(xd), xin_up, L.ptr(sd), 2, 0.2, L.ptr(out),
                   L.current_stream_ptr()), "modulate")
        return out.double().cpu()
    lib = L.lib()
    e32 = float((run(lib.sln_spade_modulate_up, L.ptr(wgb)) - ref).abs().max())
    e1 = float((run(lib.sln_spade_modulate_up_f16, L.ptr(hi), None) - ref_r).abs().max())
    e3 = float((run(lib.sln_spade_modulate_up_f16, L.ptr(hi), L.ptr(lo)) - ref).abs().max())
    bound = 2 * e32 + 1e-6
    assert e1 <= bound, ("one product vs fp64 of the fp16-rounded operands", e1, "bound", bound)
    assert e3 <= bound, ("three products vs fp64 of the unrounded operands", e3, "bound", bound)


def test_f16_entry_points_refuse_bad_sizes():
    L = pkg("_lib")
    lib = L.lib()
    x = torch.zeros(1, 16, 8, 8, device="cuda"); y = torch.zeros(1, 64, 8, 8, device="cuda")
    h = torch.zeros(1, 9, 64, 16, dtype=torch.float16, device="cuda"); b = torch.zeros(64, device="cuda")
    st = L.current_stream_ptr()
    assert lib.sln_spade_conv_f16(L.ptr(x), 1, 16, 8, 8, L.ptr(h), None, L.ptr(b), 64, 64, 1, 0, 0.0, L.ptr(y), st) == -2     # 1x1
    assert lib.sln_spade_conv_f16(L.ptr(x), 1, 16, 8, 8, None, None, L.ptr(b), 64, 64, 3, 0, 0.0, L.ptr(y), st) == -1
    assert lib.sln_spade_conv_f16(L.ptr(x), 1, 16, 8, 8, L.ptr(h), None, L.ptr(b), 64, 60, 3, 0, 0.0, L.ptr(y), st) == -1      # rows_pad
    assert lib.sln_spade_modulate_up_f16(L.ptr(x), 1, 16, 7, 8, L.ptr(h), None, L.ptr(b), 32, 64, L.ptr(x), 1, L.ptr(b), 0, 0.0,
                                         L.ptr(y), st) == -1                                                                     # odd H, xin_up


def _bench_generator():
    S = pkg("host.SPADE_related")
    from oracle.gen_golden_spade import BENCH_IMG_GAIN, BENCH_SEED
    torch.manual_seed(BENCH_SEED)
    G = S.SPADEGenerator4(41, 3, 256, 64, 'spectralspadelayer3x3', 256, 'normal')
    with torch.no_grad():
        G.conv_img.weight.mul_(BENCH_IMG_GAIN); G.conv_img.bias.mul_(BENCH_IMG_GAIN)
    syn = pkg("host.synthetic")
    seg, z = syn.spade_input(2, seed=BENCH_SEED)
    return G.cuda().eval(), seg, z


def _oracle64(G, seg, z):
    sd = {k: v.detach().cpu().double() for k, v in G.state_dict().items()}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        return spade_ref.generator(sd, spade_ref.SpadeConfig(), seg.double(), z.double())


def test_f16x3_generator_at_the_bench_weights_within_1e4_of_the_fp64_oracle():
    """The bars of the fp32 path's bench-weight test, in the three-product mode: the reference-generated spade_bench fixture (crop,
    rows, every block's checksum) and the fp64 oracle, each within 1e-4."""
    G, seg, z = _bench_generator()
    G.conv_precision = "f16x3"
    taps = {}
    with torch.no_grad():
        out = G(seg.cuda(), z.cuda()).cpu()
        out0 = G(seg[:1].cuda(), z[:1].cuda(), taps=taps).cpu()
    g = load_golden("spade_bench")
    scale = float(np.abs(g["out_rows"]).max())
    e_crop = float(np.abs(out0[:, :, 100:132, 60:92].numpy() - g["out_crop"]).max()) / scale
    e_rows = float(np.abs(out0[:, :, ::37, :].numpy() - g["out_rows"]).max()) / scale
    assert max(e_crop, e_rows) <= 1e-4, ("f16x3 vs the reference's own fp32 output", e_crop, e_rows)
    for n, t in taps.items():
        assert_close(np.array([t.double().abs().sum().item(), (t.double() ** 2).sum().item()]), g["check:" + n][1:], "f16x3:" + n, rtol=1e-4)
    r64 = _oracle64(G, seg, z)
    for b in range(2):
        e = float((out[b].double() - r64[b]).abs().max()) / float(r64[b].abs().max())
        assert e <= 1e-4, (b, e, "f16x3 vs the fp64 oracle (1e-4)")


def test_f16_generator_within_twice_the_cpu_budget():
    """One product per term: image error against the fp64 oracle and save_color bytes against the fp32 path within 2x what the CPU
    emulation of the same rounding gives at the same weights (tools/spade_half_budget.py BUDGET['bench']['f16'])."""
    budget = _budget().BUDGET["bench"]["f16"]
    G, seg, z = _bench_generator()
    I = pkg("host.spade_input")
    with torch.no_grad():
        ref32 = G(seg.cuda(), z.cuda())
        G.conv_precision = "f16"
        out = G(seg.cuda(), z.cuda())
    r64 = _oracle64(G, seg, z)
    e = max(float((out[b].double().cpu() - r64[b]).abs().max()) / float(r64[b].abs().max()) for b in range(2))
    u_16, u_32 = I.to_uint8(out).cpu().int(), I.to_uint8(ref32).cpu().int()
    share = float((u_16 != u_32).double().mean())
    maxd = int((u_16 - u_32).abs().max())
    assert e <= 2 * budget["max_err"], "f16 image vs fp64 oracle: %.2e > 2 x CPU budget %.2e" % (e, budget["max_err"])
    assert share <= 2 * budget["bytes_differ"], "f16 save_color bytes differing from fp32: %.4f > 2 x CPU budget %.4f" % (share, budget["bytes_differ"])
    assert maxd <= 2 * budget["max_byte_diff"], "f16 largest byte difference %d > 2 x CPU budget %d" % (maxd, budget["max_byte_diff"])


def test_mode_switching_keeps_no_stale_state_and_every_path_honours_the_mode():
    """fp32 -> f16 -> f16x3 -> fp32 on one module: the fp32 images are bit-identical to a fresh module's; in every mode the batch
    equals per-sample calls, one map with many z equals the broadcast, and repeated batch-1 calls on one map (kept planes, with and
    without the captured graph) equal the first, eager one."""
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    G = _gen(cfg, 7)
    seg, z = [t.cuda() for t in spade_ref.synth_input(cfg, 4, seed=3)]
    # schedules that sum in another order (batch-1 input-channel split, kept planes) differ in the last bits of an fp32 activation;
    # in the one-product mode such a difference can move its fp16 rounding by one step: that mode's tolerance is its own budget
    tol = dict(fp32=2e-4, f16x3=2e-4, f16=2 * _budget().BUDGET["bench"]["f16"]["max_err"])
    with torch.no_grad():
        fresh = _gen(cfg, 7)(seg, z)
        images = {}
        for mode in ("fp32", "f16", "f16x3", "fp32"):
            G.conv_precision = mode
            out = G(seg, z)
            if mode == "fp32":
                assert torch.equal(out, fresh), "fp32 after a half mode differs from a fresh module"
            else:
                assert float((out - fresh).abs().max()) > 0, mode           # the mode is in effect
            images[mode] = out
            for b in (0, 3):
                one = G(seg[b:b + 1].contiguous(), z[b:b + 1].contiguous())
                assert_close(out[b:b + 1].cpu().numpy(), one.cpu().numpy(), "%s: sample %d" % (mode, b), rtol=0, atol=tol[mode])
            shared = G(seg[1:2].contiguous(), z)
            per = G(seg[1:2].expand(4, -1, -1, -1).contiguous(), z)
            assert_close(shared.cpu().numpy(), per.cpu().numpy(), "%s: shared vs broadcast" % mode, rtol=0, atol=tol[mode])
            m = seg[2:3].contiguous()
            eager = [G(m, z[k:k + 1].contiguous()).clone() for k in range(4)]
            try:
                G.graph_batch1 = True
                G.clear_map_cache()
                graphed = [G(m, z[k:k + 1].contiguous()).clone() for k in range(4)]
            finally:
                G.graph_batch1 = False
                G.clear_map_cache()
            first = G(m, z[:1].contiguous())
            for k in range(4):
                assert_close(graphed[k].cpu().numpy(), eager[k].cpu().numpy(), "%s: graph_batch1 call %d" % (mode, k), rtol=0, atol=tol[mode])
            assert_close(eager[0].cpu().numpy(), first.cpu().numpy(), "%s: kept planes vs fresh map" % mode, rtol=0, atol=tol[mode])
        assert float((images["f16"] - images["f16x3"]).abs().max()) > 0
    G.conv_precision = "bf16"
    with pytest.raises(ValueError):
        G(seg, z)


@pytest.mark.parametrize("mode", ["f16", "f16x3"])
def test_deterministic_mode_is_bit_identical_in_the_half_modes(mode):
    L = pkg("_lib")
    cfg = spade_ref.SpadeConfig(ngf=16, nz=16, crop_size=128)
    G = _gen(cfg, 5)
    G.conv_precision = mode
    seg, z = [t.cuda() for t in spade_ref.synth_input(cfg, 3, seed=4)]
    try:
        L.lib().sln_set_deterministic(1)
        runs = [G(seg, z).clone() for _ in range(3)]
        shared = [G(seg[:1].contiguous(), z).clone() for _ in range(2)]
        ones = [G(seg[:1].contiguous(), z[:1].contiguous()).clone() for _ in range(3)]
    finally:
        L.lib().sln_set_deterministic(0)
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    assert torch.equal(shared[0], shared[1])
    assert torch.equal(ones[1], ones[2])


def test_captured_batch1_graph_survives_a_mode_round_trip():
    """graph_batch1 in "f16": the third call on a map captures the call (the f16 pack's addresses recorded).  A switch to "fp32" with a
    batched call repacks and drops that pack; blocks of its size are then handed out again and overwritten.  Back in "f16" the key of
    the captured call matches again and it is replayed: it must still read the weights it was captured with."""
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    G = _gen(cfg, 7)
    seg, z = [t.cuda() for t in spade_ref.synth_input(cfg, 4, seed=3)]
    m = seg[2:3].contiguous()
    with torch.no_grad():
        G.conv_precision = "f16"
        eager = [G(m, z[k:k + 1].contiguous()).clone() for k in range(4)]          # eager reference (kept planes from call 2 on)
        G.clear_map_cache()
        try:
            G.graph_batch1 = True
            first = [G(m, z[k:k + 1].contiguous()).clone() for k in range(3)]       # call 3 is captured and replayed
            assert G._b1_graph is not None and G._b1_graph["graph"] is not None
            G.conv_precision = "fp32"
            G(seg, z)                                                              # repacks: the f16 pack is released
            sizes = sorted({t.numel() for e in G._b1_graph["packed"].values() if isinstance(e, dict)
                            for v in e.values() if isinstance(v, tuple) and v and torch.is_tensor(v[0]) for t in v if torch.is_tensor(t)})
            junk = [torch.full((n,), 1e4, dtype=torch.float16, device="cuda") for n in sizes for _ in range(4)]
            G.conv_precision = "f16"
            again = [G(m, z[k:k + 1].contiguous()).clone() for k in (3, 0)]
            del junk
        finally:
            G.graph_batch1 = False
            G.clear_map_cache()
    tol = 2 * _budget().BUDGET["bench"]["f16"]["max_err"]
    for k in range(3):
        assert_close(first[k].cpu().numpy(), eager[k].cpu().numpy(), "capture call %d" % k, rtol=0, atol=tol)
    assert_close(again[0].cpu().numpy(), eager[3].cpu().numpy(), "replay after f16 -> fp32 -> f16", rtol=0, atol=tol)
    assert_close(again[1].cpu().numpy(), eager[0].cpu().numpy(), "replay after f16 -> fp32 -> f16, z 0", rtol=0, atol=tol)


@pytest.mark.parametrize("mode", ["f16", "f16x3"])
def test_nan_activations_propagate_in_the_half_modes(mode):
    """A NaN in the input stays NaN in the outputs whose 3x3 window holds it (as on the fp32 path), not finite garbage."""
    L = pkg("_lib"); S = pkg("host.SPADE_related")
    g = torch.Generator().manual_seed(3)
    B, Cin, Cout, H, W = 1, 32, 64, 16, 16
    x = torch.randn(B, Cin, H, W, generator=g)
    x[0, 5, 7, 9] = float("nan")
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    wp, rp = S._pack(w.cuda())
    hi, lo = S.split_f16(wp)
    bp = torch.zeros(rp, device="cuda")
    y = torch.empty(B, Cout, H, W, device="cuda")
    L.check(L.lib().sln_spade_conv_f16(L.ptr(x.cuda()), B, Cin, H, W, L.ptr(hi), L.ptr(lo) if mode == "f16x3" else None, L.ptr(bp), Cout, rp,
                                       3, 0, 0.0, L.ptr(y), L.current_stream_ptr()), "conv")
    nan = torch.isnan(y.cpu())
    assert bool(nan[0, :, 6:9, 8:11].all())
    assert int(nan.sum()) == Cout * 9
