"""The refinement loss under a validity mask, the parts that need no GPU: the pooled mask's tap-set restatement against a
brute-force loop over pool_kernel's index expressions, the property that an invalid image pixel is addressed by invalid pooled pixels
only (against the backward kernels' own CSR tables), ``refinement_loss_masked`` - the torch statement of the definition, the yardstick of
tests/test_refine_mask_gpu.py - and the argument checks."""
import types

import numpy as np
import pytest
import torch

import refine_mask_cases as MC
from conftest import pkg


@pytest.mark.parametrize("S", sorted(MC.GEOMETRIES))
def test_tap_set_restatement_equals_the_brute_force_loop(S):
    R = pkg("host.refine")
    sizes = MC.GEOMETRIES[S]
    tables = MC.stage_tables(R._bilinear_taps, S, sizes)
    pats = MC.patterns(S)
    got = R.valid_pooled_torch(torch.from_numpy(np.stack([pats[n] for n in MC.PATTERNS])), sizes).numpy()
    for k, name in enumerate(MC.PATTERNS):
        want = MC.brute_force_valid_pooled(pats[name], tables, sizes)
        assert np.array_equal(got[k], want), name
        print("S = %d %-12s valid pooled pixels per scale: %s" % (S, name, want.sum(axis=(1, 2)).tolist()))
    at = {n: k for k, n in enumerate(MC.PATTERNS)}
    assert got[at["ones"]].all() and not got[at["zeros"]].any()
    assert not got[at["checkerboard"]].any(), "the checkerboard must pool to all-invalid at every scale"
    for name in ("corner00", "cornerSS", "interior"):                  # conservative by at most one pixel: a few pooled pixels per scale
        lost = (~got[at[name]]).sum(axis=(1, 2))
        # (align_corners=True addresses the corners at every scale; a coarse scale may step over an interior pixel altogether)
        assert (lost <= 36).all() and lost[-1] >= 1 and (name == "interior" or (lost >= 1).all()), (name, lost)


@pytest.mark.parametrize("S", sorted(MC.GEOMETRIES))
def test_an_invalid_image_pixel_is_addressed_by_invalid_pooled_pixels_only(S):
    """against col_ptr / col_out of RefineLoss._build_tables - the lists the backward kernels gather through"""
    R = pkg("host.refine")
    sizes = MC.GEOMETRIES[S]
    P = sizes[-1]
    keep, _ = R.RefineLoss._build_tables(S, sizes, "cpu")
    col_ptr, col_out = keep[6].numpy(), keep[7].numpy()
    pats = MC.patterns(S)
    vp = R.valid_pooled_torch(torch.from_numpy(np.stack([pats[n] for n in MC.PATTERNS])), sizes).numpy()
    for s in range(len(sizes)):
        A = np.zeros((P, S))                                           # A[o, i] = 1: pooled index o reads image index i with a weight != 0
        for i in range(S):
            A[col_out[col_ptr[s, i]:col_ptr[s, i + 1]], i] = 1.0
        assert (A.sum(1) >= 1).all()
        for k, name in enumerate(MC.PATTERNS):
            reach = A @ (pats[name] == 0).astype(np.float64) @ A.T > 0     # pooled pixels that read some invalid image pixel
            assert not (reach & vp[k, s]).any(), (name, s)


def _images(S=96, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(B, 70, S, S, generator=g, dtype=torch.float64)
    target[:, 1:41] = (target[:, 1:41] > 0.9).double()
    target[:, 1:41, :7, :9] = 0.0                                      # a corner without any class: labels of -100 in the unmasked loss too
    img = (target + 0.1 * torch.randn(B, 70, S, S, generator=g, dtype=torch.float64)).clamp(0, 1)
    return target, img


def test_all_ones_mask_equals_the_unmasked_loss():
    R = pkg("host.refine")
    target, img = _images()
    labels = R.target_labels(target)
    size_loss = torch.tensor(0.37, dtype=torch.float64)
    want = R.refinement_loss(img, target, labels, size_loss)
    got = R.refinement_loss_masked(img, target, labels, size_loss, torch.ones(2, 96, 96, dtype=torch.uint8))
    for a, b in zip(got, want):
        assert abs(float(a) - float(b)) <= 1e-12 * max(abs(float(b)), 1.0), (float(a), float(b))


@pytest.mark.parametrize("name", ["rectangle", "random", "corner00", "row"])
def test_content_under_the_mask_reaches_neither_value_nor_gradient(name):
    R = pkg("host.refine")
    target, img = _images()
    valid = torch.from_numpy(np.stack([MC.pattern(name, 96), MC.pattern("interior", 96)]))
    hole = (valid == 0)[:, None].expand_as(target)
    labels = R.target_labels(torch.where(hole, torch.zeros_like(target), target))
    out = []
    for fill in (None, float("nan"), 1e30):
        t = target.clone()
        if fill is not None:
            t[hole] = fill
        x = img.clone().requires_grad_(True)
        loss, depth, sem = R.refinement_loss_masked(x, t, labels, torch.zeros((), dtype=torch.float64), valid)
        loss.backward()
        out.append((loss.detach(), depth.detach(), sem.detach(), x.grad))
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())
        assert float(x.grad[:, 1:][hole[:, 1:]].abs().max()) == 0.0       # exactly 0 on every invalid pixel of planes 1..69
        assert float(x.grad.abs().max()) > 0.0
    for other in out[1:]:
        for a, b in zip(other, out[0]):
            assert torch.equal(a, b)
    # and the mask matters: the unmasked loss of the same clean images is another number
    assert float(R.refinement_loss(img, target, R.target_labels(target), torch.zeros((), dtype=torch.float64))[1]) != float(out[0][1])


def test_all_zeros_mask():
    R = pkg("host.refine")
    target, img = _images(B=1)
    x = img.clone().requires_grad_(True)
    t = target.clone()
    t[:] = float("nan")
    labels = R.target_labels(torch.zeros_like(target))
    loss, depth, sem = R.refinement_loss_masked(x, t, labels, torch.zeros((), dtype=torch.float64), torch.zeros(1, 96, 96, dtype=torch.uint8))
    assert float(loss.detach()) == 0.0 and float(depth.detach()) == 0.0 and float(sem.detach()) == 0.0
    loss.backward()
    assert float(x.grad.abs().max()) == 0.0


def test_mask_counts_restatement():
    """the counts sln_refine_loss_mask is held to (mask_counts_torch): per room and over the batch"""
    R = pkg("host.refine")
    valid = torch.from_numpy(np.stack([MC.pattern("rectangle", 96), MC.pattern("zeros", 96)]))
    labels = torch.zeros(2, 4, 96, 96, dtype=torch.int32)
    labels[:, 1] = -100
    room = R.mask_counts_torch(valid, labels, True)
    assert room["mask_status"].tolist() == [2, 3]
    assert room["depth_count"][1].tolist() == [int(valid[0].sum()), 0] and room["depth_count"][0, 1] == 0
    assert room["depth_count"][0, 0] == int(R.valid_pooled_torch(valid[:1]).sum())
    assert torch.isinf(room["inv_count"][0, 1]) and float(room["inv_count"][0, 0]) == float(np.float32(1.0) / np.float32(int(room["valid_pooled"][0, 0].sum())))
    batch = R.mask_counts_torch(valid, labels, False)
    assert batch["mask_status"].tolist() == [2, 2] and batch["depth_count"][0].tolist() == [int(room["depth_count"][0, 0])] * 2
    assert batch["inv_count"].shape == (4,) and bool((batch["labels"][1] == -100).all())


def test_refused_mask_arguments():
    R = pkg("host.refine")
    ok = torch.ones(2, 8, 8, dtype=torch.uint8)
    R.check_mask(None, (2, 8, 8), "cpu", None)
    R.check_mask(ok, (2, 8, 8), "cpu", None)
    R.check_mask(ok.bool(), (2, 8, 8), "cpu", None)
    R.check_mask("readings", (2, 8, 8), "cpu", (None, None))
    for bad in ("readings", "holes", ok[:1], ok[:, :4], ok.float(), ok.to(torch.int32), ok.numpy(), 1):
        with pytest.raises(ValueError):
            R.check_mask(bad, (2, 8, 8), "cpu", None)
    # RefineBatch refuses in front of its first launch: a stand-in model is all it has touched by then
    model = types.SimpleNamespace(flat_params=torch.zeros(1))
    rooms = [dict(class_names=["bed", "__room__"])] * 2
    for bad in ("readings", "holes", ok, torch.ones(2, 16, 16), torch.ones(3, 16, 16, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            R.RefineBatch(model, rooms, image_size=16, mask=bad)
    with pytest.raises(ValueError):
        R.finetune_vae(None, None, None, torch.zeros(2, 6), None, None, ["bed", "__room__"], image_size=16, mask="readings")
    with pytest.raises(ValueError):
        R.finetune_vae(None, None, None, torch.zeros(2, 6), None, None, ["bed", "__room__"], image_size=16, mask=torch.ones(8, 8, dtype=torch.uint8))
