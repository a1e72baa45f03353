"""The refinement loss under a per-pixel confidence of the target, the parts that need no GPU: the pooled confidence's
tap-set restatement against a brute-force 16-tap minimum, ``refinement_loss_confidence`` - the torch statement of the definition, the
yardstick of tests/test_refine_conf_gpu.py - against ``refinement_loss_masked`` where the two must coincide, the counts the set-up call
is held to against plain loops, the argument checks and ``ObservedFuser.confidence``'s formula."""
import types

import numpy as np
import pytest
import torch

import refine_conf_cases as CC
import refine_mask_cases as MC
from conftest import pkg


@pytest.mark.parametrize("S", sorted(CC.GEOMETRIES))
def test_tap_set_minimum_equals_the_brute_force_loop(S):
    R = pkg("host.refine")
    sizes = CC.GEOMETRIES[S]
    tables = MC.stage_tables(R._bilinear_taps, S, sizes)
    pats = CC.patterns(S)
    conf = torch.from_numpy(np.stack([pats[n] for n in CC.PATTERNS]))
    got = R.conf_pooled_torch(conf, sizes)
    assert got.dtype == torch.uint8
    # the support of the pooled confidence is the pooled validity of the mask conf != 0
    assert torch.equal(got != 0, R.valid_pooled_torch(conf, sizes))
    for k, name in enumerate(CC.PATTERNS):
        want = CC.brute_force_conf_pooled(pats[name], tables, sizes)
        assert np.array_equal(got[k].numpy(), want), name
        print("S = %d %-7s pooled mean per scale %s, zeros per scale %s" % (S, name, want.mean(axis=(1, 2)).round(1).tolist(),
                                                                          (want == 0).sum(axis=(1, 2)).tolist()))
    at = {n: k for k, n in enumerate(CC.PATTERNS)}
    assert bool((got[at["full"]] == 255).all()) and not bool(got[at["zeros"]].any()) and bool((got[at["ramp"]] > 0).all())
    assert torch.equal(got[at["binary"]], R.valid_pooled_torch(torch.from_numpy(MC.pattern(CC.BINARY_MASK, S))[None], sizes)[0].to(torch.uint8) * 255)
    for name in CC.GRADED:                                             # graded where it counts: several levels survive the minimum
        assert len(set(got[at[name]].unique().tolist()) - {0}) >= 2, name


def _images(S=96, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(B, 70, S, S, generator=g, dtype=torch.float64)
    target[:, 1:41] = (target[:, 1:41] > 0.9).double()
    target[:, 1:41, :7, :9] = 0.0                                      # a corner without any class: labels of -100 without any confidence too
    img = (target + 0.1 * torch.randn(B, 70, S, S, generator=g, dtype=torch.float64)).clamp(0, 1)
    return target, img


_CACHE = {}


def _shared():
    """the images, built once and never modified"""
    if "im" not in _CACHE:
        _CACHE["im"] = _images()
    return _CACHE["im"]


def _value_and_gradient(fn, img, *args):
    x = img.clone().requires_grad_(True)
    out = fn(x, *args)
    out[0].backward()
    return [float(o.detach()) for o in out], x.grad


def _close(a, b, rel=1e-12):
    return abs(a - b) <= rel * max(abs(b), 1e-300)


def test_a_binary_confidence_is_the_masked_loss():
    R = pkg("host.refine")
    target, img = _shared()
    valid = torch.from_numpy(np.stack([MC.pattern("rectangle", 96), MC.pattern("random", 96)]))
    labels = R.target_labels(torch.where((valid != 0)[:, None], target, torch.zeros_like(target)))
    size_loss = torch.tensor(0.37, dtype=torch.float64)
    want, gw = _value_and_gradient(R.refinement_loss_masked, img, target, labels, size_loss, valid)
    got, gg = _value_and_gradient(R.refinement_loss_confidence, img, target, labels, size_loss, valid * 255)
    print("binary confidence %s, masked %s, largest gradient difference %.3g of %.3g" % (got, want, float((gg - gw).abs().max()), float(gw.abs().max())))
    assert all(_close(a, b) for a, b in zip(got, want)), (got, want)
    assert float((gg - gw).abs().max()) <= 1e-12 * float(gw.abs().max()) and float(gw.abs().max()) > 0
    # all 255: the unmasked loss
    full = torch.full((2, 96, 96), 255, dtype=torch.uint8)
    want = [float(x) for x in R.refinement_loss(img, target, R.target_labels(target), size_loss)]
    got = [float(x) for x in R.refinement_loss_confidence(img, target, R.target_labels(target), size_loss, full)]
    assert all(_close(a, b) for a, b in zip(got, want)), (got, want)


def test_a_constant_confidence_cancels():
    """each image is normalised by its own sum of weights: a constant 51 on the mask's support is the mask"""
    R = pkg("host.refine")
    target, img = _shared()
    valid = torch.from_numpy(np.stack([MC.pattern("rectangle", 96), MC.pattern("random", 96)]))
    labels = R.target_labels(torch.where((valid != 0)[:, None], target, torch.zeros_like(target)))
    zero = torch.zeros((), dtype=torch.float64)
    want, gw = _value_and_gradient(R.refinement_loss_masked, img, target, labels, zero, valid)
    got, gg = _value_and_gradient(R.refinement_loss_confidence, img, target, labels, zero, valid * 51)
    print("constant 51: %s, mask %s, relative difference of the loss %.3g" % (got, want, abs(got[0] - want[0]) / want[0]))
    assert all(_close(a, b) for a, b in zip(got, want)), (got, want)
    assert float((gg - gw).abs().max()) <= 1e-12 * float(gw.abs().max())
    # ... while a graded one is another loss on the same support
    ramp = torch.from_numpy(CC.pattern("ramp", 96))[None] * (valid != 0).to(torch.uint8)
    graded = [float(x) for x in R.refinement_loss_confidence(img, target, labels, zero, ramp)]
    assert not _close(graded[1], want[1], 1e-6) and not _close(graded[2], want[2], 1e-6)


@pytest.mark.parametrize("name", ["blocks", "fused"])
def test_content_under_zero_confidence_reaches_neither_value_nor_gradient(name):
    R = pkg("host.refine")
    target, img = _shared()
    conf = torch.from_numpy(np.stack([CC.pattern(name, 96), CC.pattern("binary", 96)]))
    hole = (conf == 0)[:, None].expand_as(target)
    assert bool(hole.any())
    labels = R.target_labels(torch.where(hole, torch.zeros_like(target), target))
    out = []
    for fill in (None, float("nan"), float("inf"), 1e30):
        t = target.clone()
        if fill is not None:
            t[hole] = fill
        (loss, depth, sem), g = _value_and_gradient(R.refinement_loss_confidence, img, t, labels, torch.zeros((), dtype=torch.float64), conf)
        out.append((loss, depth, sem, g))
        assert np.isfinite([loss, depth, sem]).all() and bool(torch.isfinite(g).all())
        assert float(g[:, 1:][hole[:, 1:]].abs().max()) == 0.0           # exactly 0 on every pixel without confidence, planes 1..69
        assert float(g.abs().max()) > 0.0
    for other in out[1:]:
        assert other[:3] == out[0][:3] and torch.equal(other[3], out[0][3])


def test_all_zeros_confidence():
    R = pkg("host.refine")
    target, img = _shared()
    t = torch.full_like(target[:1], float("nan"))
    labels = R.target_labels(torch.zeros_like(target[:1]))
    (loss, depth, sem), g = _value_and_gradient(R.refinement_loss_confidence, img[:1], t, labels, torch.zeros((), dtype=torch.float64),
                                                torch.zeros(1, 96, 96, dtype=torch.uint8))
    assert loss == 0.0 and depth == 0.0 and sem == 0.0 and float(g.abs().max()) == 0.0


def test_the_fp32_restatement_stays_inside_the_device_tests_rule():
    """the rule tests/test_refine_conf_gpu.py holds the kernels to - values within 1e-4 |ref| + 1e-7, gradient outliers (beyond 1e-4 of the
    largest entry) at most max(4 x the fp32 restatement's share, 1e-5) - is one float32 arithmetic itself meets on the graded patterns"""
    R = pkg("host.refine")
    target, img = _shared()
    zero = torch.zeros(())
    for name in CC.GRADED:
        conf = torch.from_numpy(np.stack([CC.pattern(name, 96), CC.pattern("ramp", 96)]))
        labels = R.target_labels(torch.where((conf != 0)[:, None], target, torch.zeros_like(target)))
        v64, g64 = _value_and_gradient(R.refinement_loss_confidence, img, target, labels, zero.double(), conf)
        v32, g32 = _value_and_gradient(R.refinement_loss_confidence, img.float(), target.float(), labels, zero, conf)
        scale = float(g64.abs().max())
        share = float(((g32.double() - g64).abs() > 1e-4 * scale).double().mean())
        print("%-7s fp32 against fp64: values %s / %s, gradient outlier share %.3g, largest error %.3g of %.3g" % (
            name, v32, v64, share, float((g32.double() - g64).abs().max()), scale))
        assert all(abs(a - b) <= 1e-4 * abs(b) + 1e-7 for a, b in zip(v32, v64)), (name, v32, v64)
        # the cap is a condition on the patterns: float32's own share (sign flips of the L1 gradient at differences near 0) must leave
        # max(4 x share, 1e-5) a bound that means something - under a thousandth of the entries
        assert max(4.0 * share, 1e-5) <= 1e-3, (name, share)


def test_confidence_counts_restatement_against_plain_loops():
    R = pkg("host.refine")
    S, sizes = 40, CC.GEOMETRIES[40]
    ns, P = len(sizes), sizes[-1]
    conf = torch.from_numpy(np.stack([CC.pattern("blocks", S), CC.pattern("zeros", S), CC.pattern("ramp", S)]))
    B = conf.shape[0]
    labels = torch.from_numpy(np.random.default_rng(3).integers(0, 40, (B, ns, P, P)).astype(np.int32))
    labels[:, 1] = -100
    labels[2, :, :5] = -100
    cp = R.conf_pooled_torch(conf, sizes).numpy().astype(np.int64)
    for per_room in (True, False):
        got = R.confidence_counts_torch(conf, labels, per_room, sizes)
        assert got["conf_sum"].dtype == torch.int64 and got["depth_count"].dtype == torch.int32 and got["conf_pooled"].dtype == torch.uint8
        kept = np.zeros((B, ns), np.int64); ok = np.zeros(B, np.int64); tot = np.zeros(B, np.int64)
        for b in range(B):
            for s in range(ns):
                for y in range(P):
                    for x in range(P):
                        c = int(cp[b, s, y, x])
                        want_label = int(labels[b, s, y, x]) if c else -100
                        assert int(got["labels"][b, s, y, x]) == want_label
                        kept[b, s] += c if want_label >= 0 else 0
                        ok[b] += c != 0
                        tot[b] += c
        if not per_room:
            kept, ok, tot = np.tile(kept.sum(0), (B, 1)), np.full(B, ok.sum()), np.full(B, tot.sum())
        assert got["depth_count"][0].tolist() == ok.tolist() and got["conf_sum"][0].tolist() == tot.tolist()
        assert got["depth_count"][1].tolist() == [int((c != 0).sum()) for c in conf]
        assert got["conf_sum"][1].tolist() == [int(c.to(torch.int64).sum()) for c in conf]
        assert got["mask_status"].tolist() == [(1 if tot[b] == 0 else 0) | (2 if (kept[b] == 0).any() else 0) for b in range(B)]
        with np.errstate(divide="ignore"):
            inv = (np.float32(1.0) / (kept.astype(np.float64) / 255.0).astype(np.float32))
        inv = inv if per_room else inv[0]
        assert np.array_equal(got["inv_count"].numpy().view(np.int32), inv.astype(np.float32).view(np.int32))
    # on a {0, 255} image: the mask's counts, and its inv_count bit for bit
    binary = torch.from_numpy(CC.pattern("binary", S))[None]
    a = R.confidence_counts_torch(binary, labels[:1], True, sizes)
    m = R.mask_counts_torch(binary, labels[:1], True, sizes)
    assert torch.equal(a["depth_count"], m["depth_count"]) and torch.equal(a["labels"], m["labels"]) and a["mask_status"].tolist() == m["mask_status"].tolist()
    assert torch.equal(a["conf_pooled"], m["valid_pooled"] * 255) and a["conf_sum"][0].tolist() == [255 * int(m["depth_count"][0, 0])]
    assert np.array_equal(a["inv_count"].numpy().view(np.int32), m["inv_count"].numpy().view(np.int32))


def test_refused_confidence_arguments():
    R = pkg("host.refine")
    ok = torch.full((2, 8, 8), 200, dtype=torch.uint8)
    R.check_confidence(None, (2, 8, 8), "cpu")
    R.check_confidence(ok, (2, 8, 8), "cpu")
    R.check_confidence(None, (2, 8, 8), "cpu", mask=ok)                  # a mask alone is the mask's business
    for bad in (ok[:1], ok[:, :4], ok.float(), ok.bool(), ok.to(torch.int32), ok.numpy(), "readings", 1):
        with pytest.raises(ValueError):
            R.check_confidence(bad, (2, 8, 8), "cpu")
    with pytest.raises(ValueError):
        R.check_confidence(ok, (2, 8, 8), "meta")                        # another device
    for mask in (ok, ok.bool(), "readings"):                             # together with a mask
        with pytest.raises(ValueError):
            R.check_confidence(ok, (2, 8, 8), "cpu", mask=mask)
    with pytest.raises(ValueError):                                      # views: the V axis is missing
        R.check_confidence(ok, (2, 3, 8, 8), "cpu", views=object())
    # RefineBatch refuses in front of its first launch: a stand-in model is all it has touched by then
    model = types.SimpleNamespace(flat_params=torch.zeros(1))
    rooms = [dict(class_names=["bed", "__room__"])] * 2
    good = torch.full((2, 16, 16), 255, dtype=torch.uint8)
    for bad in (ok, good.float(), good.bool(), torch.ones(3, 16, 16, dtype=torch.uint8), "readings"):
        with pytest.raises(ValueError):
            R.RefineBatch(model, rooms, image_size=16, confidence=bad)
    with pytest.raises(ValueError):
        R.RefineBatch(model, rooms, image_size=16, confidence=good, mask=good)
    eye = torch.eye(3)[None, None].repeat(2, 3, 1, 1)
    views = (eye * 20.0 + 0.0, eye, torch.zeros(2, 3, 3))
    with pytest.raises(ValueError):                                      # [R, S, S] under views of V = 3
        R.RefineBatch(model, rooms, image_size=16, confidence=good, views=views)
    for bad in (torch.ones(8, 8, dtype=torch.uint8), good[0].float()):
        with pytest.raises(ValueError):
            R.finetune_vae(None, None, None, torch.zeros(2, 6), None, None, ["bed", "__room__"], image_size=16, confidence=bad)
    with pytest.raises(ValueError):
        R.finetune_vae(None, None, None, torch.zeros(2, 6), None, None, ["bed", "__room__"], image_size=16, confidence=good[0], mask=good[0])


def test_fuser_confidence_formula_against_a_loop():
    RP = pkg("host.reproject")
    agree = torch.arange(0, 256, dtype=torch.int32).to(torch.uint8).reshape(1, 16, 16)
    for full in (1, 2, 3, 4, 7, 255):
        out, work = torch.full((1, 16, 16), 9, dtype=torch.uint8), torch.full((1, 16, 16), -4, dtype=torch.int32)
        got = RP.confidence_from_agree(agree, full, out, work)
        assert got is out
        want = [(min(a, full) * 255 + full // 2) // full for a in range(256)]
        assert got.reshape(-1).tolist() == want, full
        assert want[0] == 0 and want[full] == 255 and all(0 < w < 255 for w in want[1:full])
    assert RP.confidence_from_agree(agree, 2, out, work).reshape(-1)[:4].tolist() == [0, 128, 255, 255]
    for full in (0, -1, 256):
        with pytest.raises(ValueError):
            RP.confidence_from_agree(agree, full, out, work)
    # the method: the fuser's agree plane through the same formula into its static buffer; refused without the plane
    fu = types.SimpleNamespace(agree=agree, _conf=out, _conf_work=work)
    assert RP.ObservedFuser.confidence(fu, full=3) is out and out.reshape(-1)[:5].tolist() == [0, 85, 170, 255, 255]
    with pytest.raises(ValueError):
        RP.ObservedFuser.confidence(types.SimpleNamespace(agree=None), 2)
    with pytest.raises(ValueError):
        RP.ObservedFuser.confidence(fu, full=0)
