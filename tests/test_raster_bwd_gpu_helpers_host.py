"""CPU checks of what the per-face GPU tests of the rasterizer rest on (raster_bwd_gpu_util.py): the comparison fails on what it
should, the operand holder refuses aliased operands, the range checks refuse an index outside its list, and the float64
restatements of texture sampling and of the projection's adjoint agree with the oracle and hold their own fp32 evaluation to half
of the allowance meant for the kernels."""
import numpy as np
import pytest
import torch

import raster_bwd_cases as rc
import raster_bwd_gpu_util as ru
from oracle import raster_ref as rr


def _planted():
    c = rc.DENSE[2]
    faces, fi, rgb, grad = rc.dense_inputs(c)
    g64, S, n, _ = rr.nmr_backward_pixel_map_f64(faces, fi, rgb, grad, rc.EPS)
    got = g64.astype(np.float32)
    live = np.argwhere((n > 0) & (np.abs(g64) > 0))
    return got, g64, S, n, tuple(live[len(live) // 2])


def test_comparison_passes_the_rounded_reference_and_fails_a_planted_error():
    got, g64, S, n, i = _planted()
    worst, where, nmax = ru.compare("planted", got, g64, S, n, "split 16")
    assert worst <= 1.0 / 8 and nmax == int(n.max())          # rounding g64 once: 2^-24 |g64| <= 2^-24 S against at least 8 of them
    bad = got.copy()
    bad[i] = np.float32(g64[i] + 2.0 * rc.sum_bound(S, n)[i])
    with pytest.raises(AssertionError, match=r"1 of \d+ elements beyond the bound.*n = %d" % int(n[i])):
        ru.compare("planted", bad, g64, S, n, "split 16")


def test_comparison_sees_a_small_face_wrong_by_all_of_itself():
    """the room of test_raster_gpu.py: an element wrong by 100 % that 1e-4 * max|grad| of the tensor does not see"""
    faces, fi, rgb, grad = rc.room_inputs()
    g64, S, n, _ = rr.nmr_backward_pixel_map_f64(faces, fi, rgb, grad, rc.EPS)
    got = g64.astype(np.float32)
    small = tuple(np.argwhere((n > 0) & (np.abs(g64) > 0.5 * S) & (np.abs(g64) < 1e-4 * np.abs(g64).max()))[0])
    bad = got.copy(); bad[small] = 0
    assert np.abs(bad - g64).max() <= 1e-4 * np.abs(g64).max()
    ru.compare("room", got, g64, S, n, "split 16")
    with pytest.raises(AssertionError, match="1 of .* beyond the bound"):
        ru.compare("room", bad, g64, S, n, "split 16")


def test_comparison_fails_on_a_non_zero_without_terms_and_on_nan():
    got, g64, S, n, _ = _planted()
    z = tuple(np.argwhere(n == 0)[0])
    bad = got.copy(); bad[z] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="without a term"):
        ru.compare("planted", bad, g64, S, n, "split 16")
    bad = got.copy(); bad[z] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        ru.compare("planted", bad, g64, S, n, "split 16")
    # the += contract: the prefill stays where no term exists, and is part of what the sum is compared with
    pre = rc.eighths(np.random.default_rng(0), g64.shape)
    ru.compare("planted", (pre.astype(np.float64) + g64).astype(np.float32), g64, S, n, "split 16", prefill=pre)
    with pytest.raises(AssertionError, match="the prefill"):
        ru.compare("planted", got, g64, S, n, "split 16", prefill=pre)


def test_operand_holder_refuses_aliases():
    a = torch.zeros(64)
    h = ru.Operands(upload=False)
    h.put("faces", a); h.put("grad", torch.zeros(64))
    h.launchable()
    h.put("rgb", a.view(8, 8))                                       # shares storage and pointer
    with pytest.raises(AssertionError, match="share a device pointer"):
        h.launchable()
    h = ru.Operands(upload=False)
    h.put("faces", a); h.put("rgb", a[16:])                          # another pointer inside the same block
    with pytest.raises(AssertionError, match="overlap"):
        h.launchable()
    h = ru.Operands(upload=False)                                    # a guarded output: the pointer passed is the inner one
    ru.guarded(h, "out", (2, 3), prefill=np.arange(6))
    assert h.addr("out") == h.t["out"].data_ptr() + 4 * ru.GUARD
    assert np.array_equal(ru.read_guarded(h, "out", (2, 3)), np.arange(6, dtype=np.float32).reshape(2, 3))
    h.t["out"][ru.GUARD + 6] = 0.0
    with pytest.raises(AssertionError, match="outside its output"):
        ru.read_guarded(h, "out", (2, 3))


def test_range_checks():
    fi = np.array([[-1, 0, 24]], np.int32)
    ru.check_index_map("fi", fi, 25)
    with pytest.raises(AssertionError, match="outside"):
        ru.check_index_map("fi", np.array([[0, 25]], np.int32), 25)         # a map holding F
    with pytest.raises(AssertionError, match="outside"):
        ru.check_index_map("fi", np.array([[-2, 0]], np.int32), 25)
    with pytest.raises(AssertionError):
        ru.check_index_map("fi", fi.astype(np.int64), 25)
    idx = np.array([0, 7, -1, 8], np.int32)
    with pytest.raises(AssertionError, match="2 entries outside"):
        ru.check_index_list("faces", idx, 8)
    ru.check_index_list("faces", idx, 8, exempt=np.array([False, False, True, True]))
    with pytest.raises(AssertionError, match="1 entries outside"):
        ru.check_index_list("faces", idx, 8, exempt=np.array([False, False, True, False]))
    for c in ru.PROJ:                                                        # the projection cases exempt exactly their planted corners
        faces, exempt = ru.proj_inputs(c)[1], ru.proj_inputs(c)[6]
        ru.check_index_list(c.name, faces, c.V, exempt=exempt)
        assert int(exempt.sum()) == (2 * c.B if c.F >= 5 else 0)
        assert ((faces == -1) | (faces == c.V)).sum() == exempt.sum()


@pytest.mark.parametrize("is_,B,ts,index_map", [(8, 1, 2, "forward"), (65, 3, 4, "forward"), (65, 1, 2, "random"), (8, 3, 4, "random")])
def test_texture_restatement_matches_the_oracle(is_, B, ts, index_map):
    """un-flipped, F_tex == F, scale 1: the float64 restatement against rr.nmr_texture_sample (a float path) within half the
    allowance, and against its own fp32 evaluation likewise; background exactly 0"""
    faces, tex, fi, w, d = ru.tex_inputs(is_, B, ts, False, index_map)
    ref, A = ru.texture_chw_ref(faces, tex, fi, w, d, ts, 1e-3, 1.0)
    tol = 0.5 * ru.TEX_C(ts) * rc.U * A
    orc = rr.nmr_texture_sample(faces, tex, fi, w, d, 1e-3)                  # [B,is,is,3], raster row order
    orc = np.flip(orc, 1).transpose(0, 3, 1, 2)
    assert (fi >= 0).mean() > 0.3 and (fi < 0).any()
    assert np.all(np.abs(orc - ref) <= tol), float((np.abs(orc - ref) / np.maximum(tol, 1e-300)).max())
    f32, _ = ru.texture_chw_ref(faces, tex, fi, w, d, ts, 1e-3, 1.0, dtype=np.float32)
    assert np.all(np.abs(f32 - ref) <= tol)
    bg = np.broadcast_to(np.flip(fi, 1)[:, None] < 0, ref.shape)
    assert np.all(ref[bg] == 0) and np.all(A[bg] == 0) and np.all(A[~bg] >= 0.5 - 1e-6)


@pytest.mark.parametrize("half,scale", [(True, 0.5), (True, 1.0), (False, 0.5)])
def test_texture_restatement_fill_back_and_scale(half, scale):
    """the fill_back form is the full form on torch.cat((tex, tex.permute(0, 1, 4, 3, 2, 5)), 1), and scale is a factor; fp32
    evaluation inside half the allowance"""
    faces, tex, fi, w, d = ru.tex_inputs(65, 3, 4, half, "random")
    ref, A = ru.texture_chw_ref(faces, tex, fi, w, d, 4, 1e-3, scale)
    full = np.concatenate([tex, tex.transpose(0, 1, 4, 3, 2, 5)], 1) if half else tex
    one, A1 = ru.texture_chw_ref(faces, full, fi, w, d, 4, 1e-3, 1.0)
    assert np.array_equal(ref, one * scale) and np.array_equal(A, A1 * scale)
    if half:
        assert (fi >= ru.TEX_F // 2).any() and (fi < ru.TEX_F // 2).any()
    f32, _ = ru.texture_chw_ref(faces, tex, fi, w, d, 4, 1e-3, scale, dtype=np.float32)
    assert np.all(np.abs(f32 - ref) <= 0.5 * ru.TEX_C(4) * rc.U * A)


@pytest.mark.parametrize("c", ru.PROJ, ids=[c.name for c in ru.PROJ])
def test_projection_adjoint_restatement(c):
    """the per-corner terms against float64 autograd of rr.project + rr.vertices_to_faces, the fp32 evaluation of the same terms
    inside half the allowance, and what the case claims about itself"""
    verts, faces, K, R, t, gout, exempt = ru.proj_inputs(c)
    g64, S, n = ru.project_bwd_ref(verts, faces, K, R, t, 512.0, 1e-9, gout)
    v = torch.from_numpy(verts).double().requires_grad_(True)
    fc = torch.from_numpy(np.where(exempt, 0, faces))
    out = rr.vertices_to_faces(rr.project(v, torch.from_numpy(K).double(), torch.from_numpy(R).double(), torch.from_numpy(t).double(),
                                          512.0, 1e-9), fc)
    (out * torch.from_numpy(np.where(exempt[..., None], 0, gout)).double()).sum().backward()
    assert np.abs(v.grad.numpy() - g64).max() <= 1e-12 * max(1.0, np.abs(g64).max())
    g32, _, _ = ru.project_bwd_ref(verts, faces, K, R, t, 512.0, 1e-9, gout, dtype=np.float32)
    assert np.all(np.abs(g32.astype(np.float64) - g64) <= ru.proj_bound(S, n, share=0.5))
    assert (n[:, c.V - 1] == 0).all() and (g64[n == 0] == 0).all()                 # the vertex no face references
    assert (np.abs(g64) <= S * (1 + 1e-12)).all()
    if c.F >= 88:
        assert n[:, 0].min() > 64 * 0.6 and (faces.reshape(c.B, -1) == 0).sum(1).min() > 64      # degree above 64, some corners' gout is zero
    assert (gout.reshape(c.B, -1, 3) == 0).all(2).any()
    n4 = {4: 3, 88: 66, 172: 129}
    assert (3 * c.F) % 4 != 0 if c.F == 5 else (3 * c.F) // 4 == n4[c.F]
