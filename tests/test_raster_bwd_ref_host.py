"""CPU checks of the rasterizer backward cases (raster_bwd_cases.py) and of their double-sum reference (oracle/raster_ref.cpp,
raster_bwd_ref.py): the reference alone stays inside half of the allowance meant for the kernels (raster_bwd_cases.sum_bound),
and every case reaches the path it is named for - read from the reference's path counters, not from a kernel."""
import numpy as np
import pytest

import raster_bwd_cases as rc
import raster_bwd_ref as rb
from oracle import raster_ref as rr


def _check_reference(name, g32, g64, S, n, faces):
    """the oracle's float path within half the kernels' allowance of the double sum; the double sum finite and well populated"""
    assert np.isfinite(g64).all() and np.isfinite(S).all(), name
    err = np.abs(g32.astype(np.float64) - g64)
    tol = rc.sum_bound(S, n, share=0.5)
    bad = np.argwhere(err > tol)
    ratio = err / np.maximum(rc.U * S, 1e-300)
    assert bad.shape[0] == 0, "%s: %d elements of the float path beyond (4 + 0.25 sqrt(n)) 2^-24 S, first %s: %.1f half-ulps of S at n = %d" % (
        name, bad.shape[0], tuple(bad[0]), ratio[tuple(bad[0])], n[tuple(bad[0])])
    assert (g32[n == 0] == 0).all(), name
    # S > 0 on at least a third of the front-facing faces - counted here over the front-facing faces whose bounding box reaches into
    # the view, which is NARROWER than "front-facing": the padding faces (up to 5 479 of 5 504) and the triangle outside the
    # view are front-facing and can own nothing
    f = faces.reshape(-1, 3, 3)
    front = ~((f[:, 2, 1] - f[:, 0, 1]) * (f[:, 1, 0] - f[:, 0, 0]) < (f[:, 1, 1] - f[:, 0, 1]) * (f[:, 2, 0] - f[:, 0, 0]))
    in_view = (f[:, :, 0].min(1) < 1) & (f[:, :, 0].max(1) > -1) & (f[:, :, 1].min(1) < 1) & (f[:, :, 1].max(1) > -1)
    live = (S.reshape(-1, 9) > 0).any(1)
    assert live[front & in_view].sum() * 3 >= (front & in_view).sum(), (name, int(live.sum()), int((front & in_view).sum()))
    return float(ratio[n > 0].max()) if (n > 0).any() else 0.0


@pytest.mark.parametrize("c", rc.DENSE, ids=[c.name for c in rc.DENSE])
def test_dense_reference_and_paths(c):
    faces, fi, rgb, grad = rc.dense_inputs(c)
    g64, S, n, cnt = rr.nmr_backward_pixel_map_f64(faces, fi, rgb, grad, rc.EPS)
    _check_reference(c.name, rr.nmr_backward_pixel_map(faces, fi, rgb, grad, rc.EPS), g64, S, n, faces)
    assert cnt["longest_walk"] == c.is_                                   # the overhanging quad's diagonal crosses every row and column
    if c.is_ >= 65:
        assert cnt["longest_walk"] > 64 and cnt["rows_ge64"] > 0 and cnt["rows_lt64"] > 0, cnt
    else:
        assert cnt["rows_lt64"] > 0 and cnt["rows_ge64"] == 0, cnt
    assert (cnt["rows_gt128"] > 0) == (c.is_ >= 130), cnt
    assert cnt["steps_off_image"] > 0 and cnt["steps_slot_unused"] > 0, cnt
    if c.index_map == "random":
        twin = c._replace(index_map="forward")
        f2, fi2, rgb2, grad2 = rc.dense_inputs(twin)
        cnt2 = rr.nmr_backward_pixel_map_f64(f2, fi2, rgb2, grad2, rc.EPS)[3]
        assert cnt["inward_rejected"] > 2 * cnt2["inward_rejected"] > 0, (cnt, cnt2)
        assert fi.min() == -1 and fi.max() == c.F - 1


def test_room_reference():
    faces, fi, rgb, grad = rc.room_inputs()
    g64, S, n, cnt = rr.nmr_backward_pixel_map_f64(faces, fi, rgb, grad, rc.EPS)
    _check_reference("room", rr.nmr_backward_pixel_map(faces, fi, rgb, grad, rc.EPS), g64, S, n, faces)
    assert cnt["rows_ge64"] > 0 and cnt["rows_lt64"] > 0


@pytest.mark.parametrize("is_", [64, 65, 130])
def test_named_faces_reach_their_paths(is_):
    """(d) alone: unused slots; (f) alone: steps skipped off the image; (e): a ratio around 1e7"""
    def counters(tris):
        faces = np.stack(tris)[None]
        fi = rr.nmr_forward(faces, is_, 0.001, 100.0)[0]
        z = np.zeros((1, is_, is_, 3), np.float32)
        return rr.nmr_backward_pixel_map_f64(faces, fi, z, z, rc.EPS)[3]
    d = counters(rc.pixel_centre_triangle(is_))
    assert d["steps_slot_unused"] >= 4, d                 # each leg's two end steps, at least
    f = counters(rc.border_and_outside())
    assert f["steps_off_image"] > 0 and f["rows_lt64"] > 0, f
    t = rc.ulp_off_triangle(is_)[0]
    hit = False
    for v in range(3):
        for a in range(2):
            p = rc._p_of(t[v, a], is_)
            hit = hit or (p != np.round(p) and abs(p - np.round(p)) < 1e-4)
    assert hit, t


@pytest.mark.parametrize("c", rc.MULTI, ids=[c.name for c in rc.MULTI])
def test_multi_reference(c):
    faces, fi, passes, grads = rc.multi_inputs(c)
    g64, S, n, cnt = rb.pixel_map_multi_f64(faces, fi, passes, grads, rc.EPS)
    _check_reference(c.name, rb.pixel_map_multi_f32(faces, fi, passes, grads, rc.EPS), g64, S, n, faces)
    if c.P == 1:              # the composition with one pass IS the dense C = 3 reference, bit for bit
        d = rr.nmr_backward_pixel_map_f64(faces, fi, rb.unflip_hwc(passes[0]), rb.unflip_hwc(grads[0]), rc.EPS)
        assert np.array_equal(g64, d[0]) and np.array_equal(S, d[1]) and np.array_equal(n, d[2])
        h = passes[0].shape[2]
        assert np.array_equal(rb.unflip_hwc(passes[0])[:, 0, :, 1], passes[0][:, 1, h - 1, :])
    if c.P == 64:
        nz = np.array([bool(p.any()) for p in passes])
        assert nz[63] and not nz[5] and not nz[17] and not nz[40:51].any() and nz.sum() >= 40
        only63 = passes[63][:, 0] != 0
        others = np.zeros_like(only63)
        for p in range(63):
            others |= passes[p][:, 0] != 0
        assert (only63 & ~others).any() and (others & ~only63).any()
        # pass 63 contributes: without it the gradient differs
        g62 = rb.pixel_map_multi_f64(faces, fi, passes[:63], grads[:63], rc.EPS)[0]
        assert np.abs(g62 - g64).max() > 0


@pytest.mark.parametrize("c", rc.DEPTH, ids=[c.name for c in rc.DEPTH])
def test_depth_reference(c):
    faces, fi, w, d, gd = rc.depth_inputs(c)
    g64, S, n = rr.nmr_backward_depth_f64(faces, fi, w, d, gd)
    _check_reference(c.name, rr.nmr_backward_depth(faces, fi, w, d, gd), g64, S, n, faces)
    owned = np.zeros((c.B, c.F), np.int64)
    for b in range(c.B):
        owned[b] = np.bincount(fi[b][fi[b] >= 0], minlength=c.F)
    assert np.array_equal(n, np.broadcast_to(owned[:, :, None, None], n.shape))         # one term per owned pixel and element
    assert (owned == 0).any()                                                            # ownerless faces leave at once
    if c.is_ >= 64:
        assert owned.max() > 64 * 8                                                      # a walk that every slice of the split of 8 shares


def test_float_entry_points_kept_their_bits():
    """tests/golden/raster_bwd_float_parent.npz holds what nmr_backward_pixel_map / nmr_backward_depth returned for the 25-face
    cases before the two functions became one templated body each (recorded from a library built from that file): the float
    entry points still return the same bits.  (One element was re-recorded later: dense-random-map-is65 [1, 15, 1, 1], whose inward scan
    limit went through a float-to-int conversion of +inf that C++ leaves undefined - LAB_NOTES section 25.)"""
    from conftest import load_golden
    gold = load_golden("raster_bwd_float_parent")
    seen = 0
    for c in rc.DENSE:
        if "dense-" + c.name in gold.files:
            assert np.array_equal(rr.nmr_backward_pixel_map(*rc.dense_inputs(c), rc.EPS), gold["dense-" + c.name]), c.name
            seen += 1
    for c in rc.DEPTH:
        if "depth-" + c.name in gold.files:
            assert np.array_equal(rr.nmr_backward_depth(*rc.depth_inputs(c)), gold["depth-" + c.name]), c.name
            seen += 1
    assert seen == len(gold.files) == 32


def test_float_entry_points_kept_their_sums():
    """the float entry points share the body of the _f64 ones: same terms, so the float sum of a short element equals the
    double sum rounded wherever it has a single term"""
    c = rc.DENSE[2]
    faces, fi, rgb, grad = rc.dense_inputs(c)
    g32 = rr.nmr_backward_pixel_map(faces, fi, rgb, grad, rc.EPS)
    g64, S, n, _ = rr.nmr_backward_pixel_map_f64(faces, fi, rgb, grad, rc.EPS)
    one = n == 1
    assert one.any() and np.array_equal(g32[one], g64[one].astype(np.float32))


def test_launcher_splits_the_cases_claim():
    """small_batch_split of raster.hip restated: the standard cases run with the scan split 16 (pixel map) / 8 (depth), the wide
    ones with none"""
    assert rc.pixel_map_scan_split(1, rc.F_STD) == 16 and rc.pixel_map_scan_split(2, rc.F_STD) == 16
    assert rc.pixel_map_scan_split(2, 5504) == 1 and rc.pixel_map_scan_split(2, 5461) == 2
    assert rc.depth_bwd_split(1, rc.F_STD) == 8 and rc.depth_bwd_split(9, rc.F_STD) == 8
    assert rc.depth_bwd_split(8, 2112) == 1 and rc.depth_bwd_split(8, 2048) == 8
    assert rc.pixel_map_scan_split(8, rc.F_STD) == 1
    assert any(c.F == 5504 and c.B == 2 for c in rc.DENSE) and any(c.F == 2112 and c.B == 8 for c in rc.DEPTH)


@pytest.mark.parametrize("c", rc.SCENE, ids=[c.name for c in rc.SCENE])
def test_scene_reference(c):
    faces, cls, gfin = rc.scene_inputs(c)
    final, g64, S, n = rb.scene_backward_f64(faces, cls, rc.SCENE_CHAN, rc.SCENE_DCH, gfin)
    _check_reference(c.name, rb.scene_backward_f64(faces, cls, rc.SCENE_CHAN, rc.SCENE_DCH, gfin, acc="f32")[1], g64, S, n, faces)
    assert (gfin != 0).reshape(c.B, 70, -1).any(2).all()                                  # a gradient in all 70 planes
    assert (cls == -1).any() and set(np.unique(cls)) == {-1, 0, 1, 2, 3}
    fiA = rr.nmr_forward(faces, c.is_, 0.1, 100.0)[0]
    fiB = rr.nmr_forward(faces, c.is_, 0.001, 100.0)[0]
    assert (fiA != fiB).any()                                                              # (g): the two passes see different winners
    for b in range(c.B):
        seen = set(np.unique(cls[b][fiB[b][fiB[b] >= 0]]))
        assert seen == {0, 1, 3}, seen                                                     # class 2 owns no pixel
        assert np.all(final[b, 41 + 1] == 1.0) and np.all(final[b, 1 + 5] == 0.0)          # ... its depth plane holds wall_max / wall_max
        assert final[b, 41 + 0].min() < final[b, 41 + 0].max()
    sem = final[:, 1:41]
    assert np.abs(sem[sem != 0] - 1.0).max() <= 2.0 ** -22            # class-pass values: 1 to within a few ulps, not multiples of 1/8


def test_scene_composition_is_the_committed_one():
    """scene_backward_f64 with float accumulation against rr.scene_render on a tiny room: image within 1e-6 max, dV within 1e-5 max"""
    import torch
    V, F, ranges, box = rr.synth_room(2, n_objects=3, target_faces=120)
    is_ = 48
    v = torch.from_numpy(V)[None].requires_grad_(True)
    f = torch.from_numpy(F)[None]
    final = rr.scene_render(v, f, ranges, torch.from_numpy(box), image_size=is_)
    gout = torch.randn(final.shape, generator=torch.Generator().manual_seed(0))
    (final * gout).sum().backward()
    # the same scene at face level: cull, class ids in the reference's order, fill_back, projection
    K, R, t = rr.get_cam_mat(torch.from_numpy(box))
    classes = sorted(ranges.keys())
    classes.remove("wall"); classes.insert(0, "wall")
    chan = np.array([rr.NYU_CLASS.index(nm.replace("_", " ")) for nm in classes], np.int32)
    dch, k = [], 0
    for nm in classes:
        dch.append(-1 if nm in ("wall", "floor", "ceiling") else k)
        k += nm not in ("wall", "floor", "ceiling")
    cls = np.full(F.shape[0], -1, np.int32)
    for ci, nm in enumerate(classes):
        for a, b in ranges[nm]:
            cls[a:b] = ci
    v2 = torch.from_numpy(V)[None].requires_grad_(True)
    zc = (torch.matmul(v2, R.transpose(1, 2)) + t)[0, :, 2].detach().numpy()
    keep = ~(zc[F] < 0.06).any(1)
    fk = torch.from_numpy(F[keep])[None]
    faces_t = rr.vertices_to_faces(rr.project(v2, K, R, t, 512), torch.cat((fk, fk[:, :, [2, 1, 0]]), 1))
    cls2 = np.concatenate([cls[keep], cls[keep]])[None]
    img, g32 = rb.scene_backward_f64(faces_t.detach().numpy(), cls2, chan, np.array(dch, np.int32), gout.numpy(), acc="f32")
    np.testing.assert_allclose(img, final.detach().numpy(), rtol=0, atol=1e-6 * float(final.detach().abs().max()))
    faces_t.backward(torch.from_numpy(g32))
    assert float(v.grad.abs().max()) > 0
    np.testing.assert_allclose(v2.grad.numpy(), v.grad.numpy(), rtol=0, atol=1e-5 * float(v.grad.abs().max()))
