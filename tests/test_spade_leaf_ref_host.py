"""tests/spade_leaf_ref.py held to things independent of it, in fp64: F.interpolate, nn.Upsample, F.conv2d over F.pad(reflect),
torch.std and the generator oracle's layernorm2d / se_block / spade4 - and, for every case of tests/spade_leaf_cases.py, the
yardstick |ref32 - ref64| alone held inside the cap the GPU suite's tolerance may not exceed.  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spade_leaf_cases as K
import spade_leaf_ref as R
from oracle import spade_ref

D64, D32 = torch.float64, torch.float32
TOL = 1e-12


def _close(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1.0) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= TOL * scale, "%s: %.3e of scale %.3e" % (what, err, scale)


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=D64)


# ------------------------------------------------------------------------------------------------ resize, upsample
def test_nearest_index_map_is_torchs_for_every_size_pair_up_to_40():
    for dt in (D32, D64):
        for n_in in range(1, 41):
            src = torch.arange(n_in, dtype=dt).view(1, 1, n_in, 1)
            for n_out in range(1, 41):
                want = F.interpolate(src, size=(n_out, 1), mode="nearest").view(-1).long()
                assert torch.equal(R.nearest_index(n_in, n_out), want), (n_in, n_out, dt)


def test_the_float_rule_is_not_the_integer_rule_at_26_to_22_and_39_to_33():
    """the two size pairs of the GPU test's nearest cases at which min(floor(dst * (float)in / out), in - 1) and dst * in // out part"""
    for n_in, n_out in ((26, 22), (39, 33)):
        assert not torch.equal(R.nearest_index(n_in, n_out), R.nearest_index_integer_rule(n_in, n_out)), (n_in, n_out)
    assert (26, 39, 22, 33) in [c[:4] for c in K.RESIZE_NEAREST] and (39, 26, 33, 22) in [c[:4] for c in K.RESIZE_NEAREST]
    differ = [(i, o) for i in range(1, 41) for o in range(1, 41)
              if not torch.equal(R.nearest_index(i, o), R.nearest_index_integer_rule(i, o))]
    assert (26, 22) in differ and (39, 33) in differ


@pytest.mark.parametrize("case", K.RESIZE_NEAREST, ids=str)
def test_resize_nearest_is_f_interpolate(case):
    Hi, Wi, Ho, Wo, BC = case
    x = _rand(2, BC, Hi, Wi, seed=Hi + Wo)
    assert torch.equal(R.resize(x, Ho, Wo, 0), F.interpolate(x, size=(Ho, Wo), mode="nearest"))


@pytest.mark.parametrize("case", K.RESIZE_BILINEAR, ids=str)
def test_resize_bilinear_is_f_interpolate(case):
    Hi, Wi, Ho, Wo, BC = case
    x = _rand(2, BC, Hi, Wi, seed=Hi + Wo)
    _close(R.resize(x, Ho, Wo, 1), F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False), "bilinear")


@pytest.mark.parametrize("H,W", [(1, 1), (1, 4), (3, 5), (8, 8), (2, 2)])
def test_upsample2x_is_nn_upsample(H, W):
    x = _rand(2, 3, H, W, seed=H * 10 + W)
    assert torch.equal(R.upsample2x(x, 0), torch.nn.Upsample(scale_factor=2, mode="nearest")(x))
    _close(R.upsample2x(x, 1), torch.nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)(x), "bilinear x2")
    assert torch.equal(R.upsample2x(x, 0), R.resize(x, 2 * H, 2 * W, 0))
    _close(R.upsample2x(x, 1), R.resize(x, 2 * H, 2 * W, 1), "x2 as a resize")


# ------------------------------------------------------------------------------------------------ depth conv + concat
@pytest.mark.parametrize("Cs,H,W,B", K.DEPTH_CONCAT)
def test_depth_concat_is_conv2d_over_reflect_pad(Cs, H, W, B):
    seg = _rand(B, Cs, H, W, seed=Cs + H); w = _rand(K.ND, 1, 3, 3, seed=1) / 3; b = _rand(K.ND, seed=2) * 0.1
    want = torch.cat([F.leaky_relu(F.conv2d(F.pad(seg[:, 0:1], (1, 1, 1, 1), mode="reflect"), w, b), 0.01), seg[:, 1:]], 1)
    _close(R.depth_concat(seg, w.reshape(K.ND, 9), b, K.ND), want, "depth_concat")
    x = _rand(B, 5, H, W, seed=3); w5 = _rand(7, 5, 3, 3, seed=4)
    _close(R.conv3x3_reflect(x, w5, None), F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w5), "conv3x3_reflect")


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("B,n", [(1, 2), (3, 231), (2, 4097)])
def test_ln_stats_and_finalize_are_torch_std(B, n):
    x = _rand(B, n, seed=n) * 1.5 + 0.7
    want = torch.stack([x.mean(1), 1.0 / (x.std(1) + 1e-5)], 1)
    _close(R.ln_stats(x, 1e-5), want, "two-pass")
    _close(R.ln_finalize(x.sum(1), (x * x).sum(1), n, 1, 1e-5), want, "one-pass, well conditioned")


def test_rep_4_is_the_statistics_of_the_nearest_upsampled_tensor():
    x = _rand(3, 3, 4, 5, seed=9) * 1.5 + 0.7
    up = F.interpolate(x, scale_factor=2, mode="nearest").reshape(3, -1)
    want = torch.stack([up.mean(1), 1.0 / (up.std(1) + 1e-5)], 1)
    _close(R.ln_stats(x, 1e-5, D64, 4), want, "two-pass, rep 4")
    flat = x.reshape(3, -1)
    _close(R.ln_finalize(flat.sum(1), (flat * flat).sum(1), flat.shape[1], 4, 1e-5), want, "one-pass, rep 4")


def test_the_one_pass_formula_stands_on_its_fp64_sums():
    """x = 50 + 0.01 randn, n = 40 * 64 * 64 (the GPU suite's conditioning case): from fp64 sums the one-pass 1 / (std + eps) is the
    two-pass one to 1e-7; from fp32 sums of the same values it is off by more than a tenth."""
    x = K.ln_input((3, K.N_MID, "cond"))
    two = R.ln_stats(x, 1e-5)[:, 1]
    one = R.ln_finalize(x.double().sum(1), (x.double() ** 2).sum(1), x.shape[1], 1, 1e-5)[:, 1]
    assert float(((one - two) / two).abs().max()) <= 1e-7
    s32 = np.cumsum(x.numpy(), axis=1, dtype=np.float32)[:, -1]
    q32 = np.cumsum(x.numpy() * x.numpy(), axis=1, dtype=np.float32)[:, -1]
    bad = R.ln_finalize(torch.from_numpy(s32), torch.from_numpy(q32), x.shape[1], 1, 1e-5)[:, 1]
    assert float(((bad - two) / two).abs().min()) > 0.1


# ------------------------------------------------------------------------------------------------ the generator oracle
def _spade_state(C, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D64)
    p = "n"
    sd = {p + ".mlp_preshared_depth.1.weight": r(16, 1, 3, 3) / 3, p + ".mlp_preshared_depth.1.bias": r(16) * 0.1,
          p + ".mlp_shared.1.weight": r(128, 56, 3, 3) / (56 * 9) ** 0.5, p + ".mlp_shared.1.bias": r(128) * 0.1}
    for nm in ("gamma", "beta"):
        sd[p + ".mlp_%s.1.weight" % nm] = r(C, 128, 3, 3) / (128 * 9) ** 0.5
        sd[p + ".mlp_%s.1.bias" % nm] = r(C) * 0.1
    return sd, p, g


def test_layernorm_is_the_oracles():
    x = _rand(3, 5, 6, 4, seed=5) * 3 + 1
    st = R.ln_stats(x, 1e-5)
    _close((x - st[:, 0].view(-1, 1, 1, 1)) * st[:, 1].view(-1, 1, 1, 1), spade_ref.layernorm2d(x), "layernorm2d")


@pytest.mark.parametrize("C", [8, 24, 264])
def test_se_scale_add_is_the_oracles_se_block(C):
    g = torch.Generator().manual_seed(C)
    dx = torch.randn(2, C, 5, 3, generator=g, dtype=D64) + 0.2; xs = torch.randn(2, C, 5, 3, generator=g, dtype=D64)
    sd = {"se.fc.0.weight": torch.randn(C // 8, C, generator=g, dtype=D64), "se.fc.2.weight": torch.randn(C, C // 8, generator=g, dtype=D64)}
    out, scale = R.se_scale_add(xs, dx, sd["se.fc.0.weight"], sd["se.fc.2.weight"])
    _close(out, xs + spade_ref.se_block(sd, "se", dx), "x_s + se_block(dx)")
    _close(R.se_scale(dx.sum((2, 3)), 15, sd["se.fc.0.weight"], sd["se.fc.2.weight"]), scale, "from pixel sums")


@pytest.mark.parametrize("C,H,W,act", [(8, 6, 8, 0), (40, 4, 12, 2), (100, 10, 10, 2)])
def test_modulate_and_spade_apply_are_the_oracles_spade4(C, H, W, act):
    sd, p, g = _spade_state(C, C)
    x = torch.randn(2, C, H, W, generator=g, dtype=D64) * 3 + 1
    seg = torch.rand(2, 41, 2 * H + 1, 2 * W + 3, generator=g, dtype=D64)
    want = spade_ref.spade4(sd, p, x, seg)
    want = F.leaky_relu(want, 0.2) if act == 2 else want
    s = R.resize(seg, H, W, 1)
    cat = R.depth_concat(s, sd[p + ".mlp_preshared_depth.1.weight"], sd[p + ".mlp_preshared_depth.1.bias"], 16)
    actv = R.conv3x3_reflect(cat, sd[p + ".mlp_shared.1.weight"], sd[p + ".mlp_shared.1.bias"]).clamp_min(0)
    stats = R.ln_stats(x, 1e-5)
    wg, bg, wb, bb = (sd[p + ".mlp_%s.1.%s" % (a, b)] for a in ("gamma", "beta") for b in ("weight", "bias"))
    _close(R.modulate(actv, wg, bg, wb, bb, x, 0, stats, act, 0.2), want, "modulate")
    # the batch-shared form: gamma | beta of ONE map in the packed row layout, junk in the rows of no channel
    gamma, beta = R.conv3x3_reflect(actv[:1], wg, bg)[0], R.conv3x3_reflect(actv[:1], wb, bb)[0]
    gb = torch.full((K.rows_pad_of(C), H, W), float("nan"), dtype=D64)
    rg, rb = R.packed_rows(C)
    assert len(set(rg.tolist()) | set(rb.tolist())) == 2 * C and int(rb.max()) < K.rows_pad_of(C)
    gb[rg], gb[rb] = gamma, beta
    want1 = spade_ref.spade4(sd, p, x, seg[:1])
    want1 = F.leaky_relu(want1, 0.2) if act == 2 else want1
    _close(R.spade_apply(x, 0, gb, stats, C, act, 0.2), want1, "spade_apply")


def test_the_read_through_upsampling_forms_equal_the_materialised_ones():
    g = torch.Generator().manual_seed(3)
    C, H, W = 8, 4, 8
    xs = torch.randn(2, C, H // 2, W // 2, generator=g, dtype=D64); dx = torch.randn(2, C, H, W, generator=g, dtype=D64)
    scale = torch.rand(2, C, generator=g, dtype=D64)
    up = F.interpolate(xs, scale_factor=2, mode="nearest")
    for m in (-1, 0, 1):
        a, sa = R.block_tail(xs, 1, dx, scale, m); b, sb = R.block_tail(up, 0, dx, scale, m)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        v = up + dx * scale[:, :, None, None]
        want = v if m < 0 else F.interpolate(v, scale_factor=2, mode="nearest" if m == 0 else "bilinear", **({} if m == 0 else {"align_corners": False}))
        _close(a, want, "block_tail up_mode %d" % m)
        _close(sa, torch.stack([want.reshape(2, -1).mean(1), 1.0 / (want.reshape(2, -1).std(1) + 1e-5)], 1), "tail statistics")
    gb = torch.randn(64, H, W, generator=g, dtype=D64); stats = R.ln_stats(up, 1e-5)
    assert torch.equal(R.spade_apply(xs, 1, gb, stats, C, 2, 0.2), R.spade_apply(up, 0, gb, stats, C, 2, 0.2))


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("family", list(K.FAMILIES))
def test_the_yardstick_alone_stays_inside_the_cap(family):
    """allowed error = 2^-23 scale + 8 |ref32 - ref64| <= 1e-5 of the tensor's maximum for every case and every compared tensor:
    a case that breaks it has badly chosen inputs (the cap is what test_spade_gpu.py already holds these entry points to)."""
    worst = (0.0, None)
    for case in K.FAMILIES[family]:
        _, refs = K.evaluate(family, case)
        for name, (r64, r32) in refs.items():
            assert r64.dtype == D64 and r32.dtype == D32 and r64.shape == r32.shape, (family, case, name)
            assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), (family, case, name)
            al, scale = K.allowed(r64.numpy(), r32.numpy())
            worst = max(worst, (al / scale, (case, name)))
            assert al <= K.CAP * scale, "%s %s %s: allowed %.3e of scale %.3e = %.3e" % (family, case, name, al, scale, al / scale)
    print("%s: largest allowed / scale %.3e at %s" % (family, worst[0], worst[1]))


def test_the_se_cases_do_not_saturate_and_the_tables_hold_what_they_claim():
    for case in K.SE:
        _, refs = K.evaluate("se_scale_add", case)
        s = refs["scale"][0]
        open_ = float(((s > 0.02) & (s < 0.98)).double().mean())
        assert open_ >= 0.8 and float(s.max() - s.min()) > 0.3, (case, open_, float(s.min()), float(s.max()))
    assert {c // 8 for c, _ in K.SE} == {1, 3, 32, 33, 128}
    assert max(b * n for b, n, _ in K.LN_STATS) * 4 <= 8 << 20
