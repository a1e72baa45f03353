"""The SPADE generator's non-convolution kernels (csrc/spade.hip) one entry point at a time through the C ABI (run with -m gpu),
against the plain fp64 reference tests/spade_leaf_ref.py at the cases of tests/spade_leaf_cases.py: sln_resize, sln_upsample2x,
sln_spade_depth_concat, sln_layernorm_stats / _finalize, sln_se_scale_add, sln_block_tail, sln_spade_apply[_up] and the fp32
modulation epilogue of sln_spade_modulate_up.

Gathers (nearest resize / upsampling, copied mask channels, untouched sentinels) are bit-exact.  Everything else:
    |got - ref64| <= 2^-23 * max|ref64| + 8 * max|ref32 - ref64|
(parity.assert_close_conditioned; the yardstick |ref32 - ref64| comes from the reference alone, and test_spade_leaf_ref_host.py holds
the whole allowance of every case to 1e-5 of the tensor's maximum).  Every check prints its err / allowed ratio before it asserts.
"""
import pytest
import torch

from conftest import pkg
from gpu_util import _lib, _sync
from parity import assert_close_conditioned, max_err
import spade_leaf_cases as K

pytestmark = pytest.mark.gpu

EPS, SENT = K.EPS, K.SENT


def _hold(got, pair, kernel, what):
    """one compared tensor: print err / allowed, then assert"""
    r64, r32 = pair[0].numpy(), pair[1].double().numpy()
    g = got.detach().double().cpu().numpy().reshape(r64.shape)
    err, _ = max_err(g, r64)
    al, scale = K.allowed(r64, r32)
    print("leaf-ratio %s %.4f   (%s: err %.3e, allowed %.3e, scale %.3e)" % (kernel, err / al, what, err, al, scale))
    assert_close_conditioned(g, r64, r32, "%s %s" % (kernel, what), rtol=K.ULP32, atol=K.ATOL, k=K.K_NOISE)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _st(L):
    return L.current_stream_ptr()


# ------------------------------------------------------------------------------------------------ sln_resize, sln_upsample2x
@pytest.mark.parametrize("case", K.RESIZE_NEAREST, ids=str)
def test_resize_nearest_is_the_float_rule_gather(case):
    """F.interpolate's index rule min(floor(dst * (float)in / out), in - 1); 26 -> 22 and 39 -> 33 are where dst * in // out differs"""
    L = _lib()
    Hi, Wi, Ho, Wo, BC = case
    inp, refs = K.evaluate("resize_nearest", case)
    src = inp["src"].cuda()
    dst = torch.full((BC, Ho, Wo), SENT, device="cuda")
    L.check(L.lib().sln_resize(L.ptr(src), BC, Hi, Wi, Ho, Wo, 0, L.ptr(dst), _st(L)), "sln_resize")
    _sync("sln_resize")
    assert _same_bits(dst.cpu(), refs["out"][1]), "nearest resize is a gather: %d elements differ" % int((dst.cpu() != refs["out"][1]).sum())


@pytest.mark.parametrize("case", K.RESIZE_BILINEAR, ids=str)
def test_resize_bilinear(case):
    L = _lib()
    Hi, Wi, Ho, Wo, BC = case
    inp, refs = K.evaluate("resize_bilinear", case)
    src = inp["src"].cuda()
    dst = torch.full((BC, Ho, Wo), SENT, device="cuda")
    L.check(L.lib().sln_resize(L.ptr(src), BC, Hi, Wi, Ho, Wo, 1, L.ptr(dst), _st(L)), "sln_resize")
    _sync("sln_resize")
    _hold(dst, refs["out"], "sln_resize", "bilinear %s" % (case,))


@pytest.mark.parametrize("case", K.UPSAMPLE, ids=str)
def test_upsample2x(case):
    L = _lib()
    H, W, mode, BC = case
    inp, refs = K.evaluate("upsample2x", case)
    x = inp["x"].cuda()
    y = torch.full((BC, 2 * H, 2 * W), SENT, device="cuda")
    L.check(L.lib().sln_upsample2x(L.ptr(x), BC, H, W, mode, L.ptr(y), _st(L)), "sln_upsample2x")
    _sync("sln_upsample2x")
    if mode == 0:
        assert _same_bits(y.cpu(), refs["out"][1]), "nearest upsampling is a gather"
    else:
        _hold(y, refs["out"], "sln_upsample2x", "bilinear %s" % (case,))


# ------------------------------------------------------------------------------------------------ sln_spade_depth_concat
@pytest.mark.parametrize("copy_masks", [0, 1])
@pytest.mark.parametrize("case", K.DEPTH_CONCAT, ids=str)
def test_depth_concat(case, copy_masks):
    """the nd depth features against the reference; the mask channels bit for bit: copies of seg[:, 1:] (copy_masks = 1) or the
    sentinel `out` was filled with (copy_masks = 0 leaves them alone)"""
    L = _lib()
    Cs, H, W, B = case
    nd = K.ND
    inp, refs = K.evaluate("depth_concat", case)
    seg, wpd, bpd = inp["seg"].cuda(), inp["wpd"].cuda(), inp["bpd"].cuda()
    out = torch.full((B, nd + Cs - 1, H, W), SENT, device="cuda")
    L.check(L.lib().sln_spade_depth_concat(L.ptr(seg), B, Cs, H, W, L.ptr(wpd), L.ptr(bpd), nd, L.ptr(out), copy_masks, _st(L)), "depth_concat")
    _sync("sln_spade_depth_concat")
    r64, r32 = refs["out"]
    _hold(out[:, :nd], (r64[:, :nd], r32[:, :nd]), "sln_spade_depth_concat", "depth features %s" % (case,))
    masks = out[:, nd:].cpu()
    want = inp["seg"][:, 1:] if copy_masks else torch.full((B, Cs - 1, H, W), SENT)
    assert _same_bits(masks, want), "mask channels, copy_masks = %d" % copy_masks


# ------------------------------------------------------------------------------------------------ sln_layernorm_stats / _finalize
def _ln_stats(L, xd, B, n):
    scratch = torch.full((16 * B,), 7.0, dtype=torch.float64, device="cuda")          # zeroed by the call
    stats = torch.full((B, 2), SENT, device="cuda")
    L.check(L.lib().sln_layernorm_stats(L.ptr(xd), B, n, EPS, L.ptr(scratch), L.ptr(stats), _st(L)), "sln_layernorm_stats")
    _sync("sln_layernorm_stats")
    return stats


@pytest.mark.parametrize("case", K.LN_STATS, ids=str)
def test_layernorm_stats(case):
    """one workgroup per sample (n <= 4096), several, and the 128-workgroup cap whose loop strides; a second finalize workgroup
    (B = 65); 50 + 0.01 randn, where the one-pass formula stands on its fp64 sums; a constant sample, whose variance clamps at 0"""
    L = _lib()
    B, n, kind = case
    inp, refs = K.evaluate("ln_stats", case)
    stats = _ln_stats(L, inp["x"].cuda(), B, n)
    if kind == "const":
        print("constant sample: the fp64 one-pass formula gives 1 / (std + eps) = %s, %.3e away from 1 / eps (relative)" % (
            refs["inv"][0].tolist(), float((refs["inv"][0] * EPS - 1).abs().max())))
    _hold(stats[:, 0], refs["mean"], "sln_layernorm_stats", "mean %s" % (case,))
    _hold(stats[:, 1], refs["inv"], "sln_layernorm_stats", "1/(std+eps) %s" % (case,))


def test_layernorm_stats_deterministic_mode():
    """at most 7 workgroups per sample store their sums to slots the finalize adds in order: two runs give the same bits, both the
    reference's"""
    L = _lib()
    B, n, _ = K.LN_STATS_DET
    inp, refs = K.evaluate("ln_stats", K.LN_STATS_DET)
    xd = inp["x"].cuda()
    try:
        L.lib().sln_set_deterministic(1)
        runs = [_ln_stats(L, xd, B, n) for _ in range(2)]
    finally:
        L.lib().sln_set_deterministic(0)
    assert _same_bits(runs[0].cpu(), runs[1].cpu())
    for r in runs:
        _hold(r[:, 0], refs["mean"], "sln_layernorm_stats(det)", "mean")
        _hold(r[:, 1], refs["inv"], "sln_layernorm_stats(det)", "1/(std+eps)")


@pytest.mark.parametrize("case", K.LN_FINALIZE, ids=str)
def test_layernorm_finalize_from_exact_sums(case):
    """rep = 4 against the two-pass statistics of the nearest-upsampled tensor; B = 65 needs a second workgroup"""
    L = _lib()
    B, rep = case
    inp, refs = K.evaluate("ln_finalize", case)
    acc = torch.zeros(B, 16, dtype=torch.float64)
    acc[:, 0], acc[:, 1] = inp["s"], inp["q"]
    acc = acc.cuda()
    stats = torch.full((B, 2), SENT, device="cuda")
    L.check(L.lib().sln_layernorm_finalize(L.ptr(acc), B, inp["n_acc"], rep, EPS, L.ptr(stats), _st(L)), "sln_layernorm_finalize")
    _sync("sln_layernorm_finalize")
    _hold(stats[:, 0], refs["mean"], "sln_layernorm_finalize", "mean %s" % (case,))
    _hold(stats[:, 1], refs["inv"], "sln_layernorm_finalize", "1/(std+eps) %s" % (case,))


# ------------------------------------------------------------------------------------------------ sln_se_scale_add
@pytest.mark.parametrize("case", K.SE, ids=str)
def test_se_scale_add(case):
    """C / 8 = 1, 3 (scalar w2 path), 32 and 128 (vector path), 33 (scalar path, second hidden-row iteration); the scale vector left
    in scratch[B * C:] and the output"""
    L = _lib()
    Cc, hw = case
    B = K.SE_B
    inp, refs = K.evaluate("se_scale_add", case)
    xs, dx, w0, w2 = (inp[k].cuda() for k in ("xs", "dx", "w0", "w2"))
    scratch = torch.full((2 * B * Cc,), SENT, device="cuda")
    out = torch.full((B, Cc, hw, 1), SENT, device="cuda")
    L.check(L.lib().sln_se_scale_add(L.ptr(xs), L.ptr(dx), B, Cc, hw, L.ptr(w0), L.ptr(w2), L.ptr(scratch), L.ptr(out), _st(L)), "sln_se_scale_add")
    _sync("sln_se_scale_add")
    _hold(scratch[B * Cc:], refs["scale"], "sln_se_scale_add", "scale %s" % (case,))
    _hold(out, refs["out"], "sln_se_scale_add", "out %s" % (case,))


# ------------------------------------------------------------------------------------------------ sln_block_tail
@pytest.mark.parametrize("case", K.TAIL, ids=str)
def test_block_tail(case):
    """Output, scale vector and statistics (stats_rep 1 and 4; `acc` pre-filled: the call clears it) of every case:
      * the phases of se_fc_kernel at 4 x 4: with gap_sums and B <= 8 the two FCs are two launches of 1, 2 and 4 workgroups per sample
        (C = 256, 264, 1024); without gap_sums the pool kernel and one workgroup per sample; B = 9 with gap_sums: one workgroup again;
      * rows of 2 and 4 pixels (the left and the right clamp of the bilinear window on one thread), one-row images, W % 4 != 0;
      * the grid caps - 512 workgroups per sample with statistics, 4096 / B without - with loops that stride;
      * xs, dx = 50 + 0.01 randn: the statistics of ill-conditioned values.
    The n4 >= 2^31 branch of the kernel's index arithmetic needs an output of 32 GB per sample: it cannot be reached at test size."""
    L = _lib()
    B, Cc, H, W, up_mode, xs_up, with_sums, with_stats, _ = case
    inp, refs = K.evaluate("block_tail", case)
    xs, dx, w0, w2 = (inp[k].cuda() for k in ("xs", "dx", "w0", "w2"))
    sums = inp["sums"].cuda() if with_sums else None
    k = 1 if up_mode < 0 else 2
    for rep in (1, 4):
        out = torch.full((B, Cc, k * H, k * W), SENT, device="cuda")
        scratch = torch.full((2 * B * Cc,), SENT, device="cuda")
        acc = torch.full((16 * B,), 7.0, dtype=torch.float64, device="cuda") if with_stats else None
        stats = torch.full((B, 2), SENT, device="cuda") if with_stats else None
        L.check(L.lib().sln_block_tail(L.ptr(xs), xs_up, L.ptr(dx), B, Cc, H, W, L.ptr(sums), L.ptr(w0), L.ptr(w2), L.ptr(scratch), up_mode,
                                       L.ptr(out), L.ptr(acc), rep, EPS, L.ptr(stats), _st(L)), "sln_block_tail")
        _sync("sln_block_tail")
        _hold(scratch[B * Cc:], refs["scale"], "sln_block_tail", "scale %s" % (case,))
        _hold(out, refs["out"], "sln_block_tail", "out %s" % (case,))
        if with_stats:
            _hold(stats[:, 0], refs["mean_rep%d" % rep], "sln_block_tail", "mean rep %d %s" % (rep, case))
            _hold(stats[:, 1], refs["inv_rep%d" % rep], "sln_block_tail", "1/(std+eps) rep %d %s" % (rep, case))


# ------------------------------------------------------------------------------------------------ sln_spade_apply[_up], modulation
@pytest.mark.parametrize("case", K.APPLY, ids=str)
def test_spade_apply(case):
    """row(c) = 64 (c / 32) + c % 32 at one, two and four row groups; the rows of no channel hold NaN: the output is finite"""
    L = _lib()
    Cc, H, W, x_up, act = case
    B = K.APPLY_B
    inp, refs = K.evaluate("spade_apply", case)
    x, gb, stats = inp["x"].cuda(), inp["gb"].cuda(), inp["stats"].cuda()
    out = torch.full((B, Cc, H, W), SENT, device="cuda")
    if x_up:
        rc = L.lib().sln_spade_apply_up(L.ptr(x), 1, L.ptr(gb), B, Cc, H, W, inp["rows_pad"], L.ptr(stats), act, 0.2, L.ptr(out), _st(L))
    else:
        rc = L.lib().sln_spade_apply(L.ptr(x), L.ptr(gb), B, Cc, H, W, inp["rows_pad"], L.ptr(stats), act, 0.2, L.ptr(out), _st(L))
    L.check(rc, "sln_spade_apply")
    _sync("sln_spade_apply")
    assert bool(torch.isfinite(out).all()), "a row of no channel was read"
    _hold(out, refs["out"], "sln_spade_apply_up" if x_up else "sln_spade_apply", "out %s" % (case,))


@pytest.mark.parametrize("case", K.MODULATE, ids=str)
def test_modulate_fp32_with_and_without_the_read_through_upsampling(case):
    """the modulation epilogue of the fp32 convolution kernels with xin_up = 0 and 1 (the f16 suite's MOD_CASES, for fp32)"""
    L = _lib(); S = pkg("host.SPADE_related")
    Cc, H, W, xin_up, act = case
    B, Cin = K.MOD_B, K.MOD_CIN
    inp, refs = K.evaluate("modulate", case)
    wgb, bgb, rpg = S._pack_gamma_beta(inp["wg"].cuda(), inp["bg"].cuda(), inp["wb"].cuda(), inp["bb"].cuda())
    actv, xin, stats = inp["actv"].cuda(), inp["xin"].cuda(), inp["stats"].cuda()
    out = torch.full((B, Cc, H, W), SENT, device="cuda")
    L.check(L.lib().sln_spade_modulate_up(L.ptr(actv), B, Cin, H, W, L.ptr(wgb), L.ptr(bgb), Cc, rpg, L.ptr(xin), xin_up, L.ptr(stats), act, 0.2,
                                          L.ptr(out), _st(L)), "sln_spade_modulate_up")
    _sync("sln_spade_modulate_up")
    _hold(out, refs["out"], "sln_spade_modulate_up", "out %s" % (case,))
