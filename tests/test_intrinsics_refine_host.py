"""Refinement of the intrinsics of the target views, host side (DESIGN §4 "Intrinsics of the target views"): the closed form of the gradient
against autograd with K as the leaf, the float32 run of the restatement against the bound the kernel is held to, the float64 update and its
helpers (``reproject.intrinsics_step_torch``, ``intrinsics_error``, ``intrinsics_move``) and what ``refine.check_intrinsics`` refuses.  No GPU:
nothing here launches."""
import numpy as np
import pytest
import torch

from conftest import pkg

import intrinsics_refine_ref as IR
import pose_refine_cases as PC

from oracle import raster_ref as rr

KEYS = ("faces", "corners", "K", "R", "t", "grad_faces", "orig_size", "proj_eps", "cull_eps")


def _cases():
    return [(which, op) for which in ("three", "away") for op in PC.host_operands(which)]


def _autograd(op):
    """fp64 autograd through raster_ref.project with K as the leaf: L = <faces of the view (fill_back copies included, culled faces zero),
    grad_faces> -> (dL/dK[0, 0], dL/dK[1, 1], dL/dK[0, 2], dL/dK[1, 2])"""
    d = torch.float64
    p = torch.from_numpy(op["corners"]).to(d)
    Rm, t = (torch.from_numpy(op[k]).to(d) for k in ("R", "t"))
    K = torch.from_numpy(op["K"]).to(d).clone().requires_grad_(True)
    faces = torch.from_numpy(op["faces"]).long()
    F = faces.shape[0]
    kept = IR.intr_grad_ref(*(op[k] for k in KEYS))[3]                 # the kernel's cull: the float32 camera z of the float32 operands
    uvz = rr.project(p[None], K[None], Rm[None], t[None, None], op["orig_size"], eps=op["proj_eps"])
    f = rr.vertices_to_faces(uvz, faces[None])[0]
    f = torch.where(torch.from_numpy(kept)[:, None, None], f, torch.zeros_like(f))
    w = torch.from_numpy(op["grad_faces"]).to(d)
    (torch.cat((f, f[:, [2, 1, 0]])) * w[:2 * F]).sum().backward()
    g = K.grad
    return torch.stack((g[0, 0], g[1, 1], g[0, 2], g[1, 2])).numpy()


def test_closed_form_is_the_autograd_gradient_in_fp64():
    seen = 0
    for which, op in _cases():
        g, S, n, kept = IR.intr_grad_ref(*(op[k] for k in KEYS))
        ref = _autograd(op)
        top = float(np.abs(ref).max())
        print("%s room %d view %d: %d of %d faces kept, max |closed form - autograd| = %.3e, largest entry %.3e" %
              (which, op["r"], op["v"], int(kept.sum()), kept.size, float(np.abs(g - ref).max()), top))
        if n == 0:
            assert not g.any() and not ref.any()
            continue
        seen += 1
        assert top > 0 and float(np.abs(g - ref).max()) <= 1e-12 * top
    assert seen >= 8


def test_float32_restatement_stays_within_half_the_kernels_bound():
    """the kernel is held to (36 + 0.5 sqrt(n)) 2^-24 S with S = sum |term|; a float32 run of the restatement (products in float32 in the kernel's
    order, sums in float64) must lie within HALF of it for every case of tests/test_place_intrinsics_gpu.py.  Measured here (LAB_NOTES
    "Intrinsics of the target views"): worst ratio 0.034 of the bound (d fx of room 1, view 0)."""
    worst = 0.0
    for which, op in _cases():
        args = tuple(op[k] for k in KEYS)
        g64, S, n, _ = IR.intr_grad_ref(*args)
        g32 = IR.intr_grad_ref(*args, dtype=np.float32)[0]
        if n == 0:
            assert not g32.any()
            continue
        ratio = np.abs(g32 - g64) / IR.intr_bound(S, n)
        print("%s room %d view %d: n = %d, |float32 - float64| / bound per element: %s" % (which, op["r"], op["v"], n, np.array2string(ratio, precision=4)))
        worst = max(worst, float(ratio.max()))
    print("worst ratio %.4f" % worst)
    assert 0 < worst <= 0.5


def _K(fx=420.0, fy=380.0, cx=250.0, cy=262.0):
    return torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def test_a_zero_step_is_the_identity_by_bits():
    RP = pkg("host.reproject")
    K = torch.stack((_K(), _K(123.456789, 0.1, -3.0, 1e-7)))
    g = torch.tensor([[1e3, -2e3, 5.0, -7.0], [0.3, 0.1, -0.0, 1e9]], dtype=torch.float64)
    for tie in (True, False):
        out = RP.intrinsics_step_torch(K, g, 0.0, 0.0, tie)
        assert out.dtype == torch.float64 and _bits(out, K)
    assert _bits(RP.intrinsics_step_torch(K.float(), g, 0.0, 0.0), K.float().double()), "the master of a float32 K is exactly its double"
    assert _bits(RP.intrinsics_step_torch(K, torch.zeros(2, 4), 1e-3, 1e-3), K), "a zero gradient moves nothing"
    K0 = K.clone()
    RP.intrinsics_step_torch(K, g, 1e-6, 1e-3)
    assert _bits(K, K0), "the argument was written"


def test_tie_focal_keeps_the_aspect_ratio():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(64):
        K = _K(*rng.uniform(100, 900, 4))
        g = torch.from_numpy(rng.standard_normal(4) * 10.0)
        out = RP.intrinsics_step_torch(K, g, 1e-5, 1e-2, True)
        r0, r1 = float(K[0, 0] / K[1, 1]), float(out[0, 0] / out[1, 1])
        worst = max(worst, abs(r1 - r0) / r0)
        assert float(out[0, 0]) != float(K[0, 0])
        assert abs(r1 - r0) <= 5 * 2.0 ** -53 * r0                     # the two products, their quotient and r0's own: four roundings of 2^-53, and second order
        # the one log-scale: both focal lengths by the same factor
        s = -1e-5 * (K[0, 0] * g[0] + K[1, 1] * g[1])
        assert abs(float(out[0, 0]) - float(K[0, 0] * torch.exp(s))) <= 1e-12 * float(K[0, 0])
        assert _bits(out[:2, 2], torch.stack((K[0, 2] - 1e-2 * g[2], K[1, 2] - 1e-2 * g[3])))
    print("worst relative change of fx / fy: %.3e" % worst)


def test_focal_lengths_stay_positive_and_finite_under_a_huge_gradient():
    RP = pkg("host.reproject")
    for tie in (True, False):
        for sign in (1.0, -1.0):
            K = RP.intrinsics_step_torch(_K(), torch.tensor([sign * 1e30, sign * 1e30, 0.0, 0.0], dtype=torch.float64), 1.0, 0.0, tie)
            f = K[[0, 1], [0, 1]]
            assert bool(torch.isfinite(f).all()) and bool((f > 0).all()), (tie, sign, f)
            # the log-scale of one step is held to FOCAL_LOG_MAX: a factor e at the most, either way
            want = torch.stack((_K()[0, 0], _K()[1, 1])) * np.exp(-sign * RP.FOCAL_LOG_MAX)
            assert float((f - want).abs().max()) <= 1e-12 * float(want.max())
            assert float(np.float32(f.min())) > 0, "the float32 rounding the table receives"
    K = _K()
    for _ in range(200):                                               # and step after step: positive for as long as float64 has numbers
        K = RP.intrinsics_step_torch(K, torch.tensor([1e30, 1e30, 0.0, 0.0], dtype=torch.float64), 1.0, 0.0)
    assert float(K[0, 0]) > 0 and float(K[1, 1]) > 0


def test_untied_the_update_is_the_two_independent_updates():
    RP = pkg("host.reproject")
    K = _K()
    g = torch.tensor([0.7, -1.3, 4.0, -2.5], dtype=torch.float64)
    both = RP.intrinsics_step_torch(K, g, 2e-5, 3e-2, False)
    only_x = RP.intrinsics_step_torch(K, g * torch.tensor([1.0, 0.0, 1.0, 0.0]), 2e-5, 3e-2, False)
    only_y = RP.intrinsics_step_torch(K, g * torch.tensor([0.0, 1.0, 0.0, 1.0]), 2e-5, 3e-2, False)
    assert _bits(both[0], only_x[0]) and _bits(both[1], only_y[1]) and _bits(only_x[1], K[1]) and _bits(only_y[0], K[0])
    assert float(both[0, 0]) == float(K[0, 0] * torch.exp(-2e-5 * (K[0, 0] * g[0]))) and float(both[1, 1]) == float(K[1, 1] * torch.exp(-2e-5 * (K[1, 1] * g[1])))
    assert float(both[0, 2]) == float(K[0, 2] - 3e-2 * g[2]) and float(both[1, 2]) == float(K[1, 2] - 3e-2 * g[3])
    assert _bits(both[2], K[2]) and float(both[0, 1]) == 0.0 and float(both[1, 0]) == 0.0
    tied = RP.intrinsics_step_torch(K, g, 2e-5, 3e-2, True)
    assert float(tied[0, 0]) != float(both[0, 0]), "tied and untied differ when the two log-gradients do"
    # batched over leading axes
    Kb = torch.stack((K, _K(300.0, 310.0, 256.0, 256.0)))[None]
    gb = torch.stack((g, -g))[None]
    out = RP.intrinsics_step_torch(Kb, gb, 2e-5, 3e-2, False)
    assert tuple(out.shape) == (1, 2, 3, 3) and _bits(out[0, 0], both)


def test_intrinsics_error_measures_what_it_says():
    RP = pkg("host.reproject")
    K = _K()
    rel, dist = RP.intrinsics_error(K, K)
    assert float(rel) == 0.0 and float(dist) == 0.0
    rel, dist = RP.intrinsics_error(_K(420.0 * 1.03, 380.0 * 0.99, 253.0, 258.0), K)
    assert abs(float(rel) - 0.03) <= 1e-12 and abs(float(dist) - 5.0) <= 1e-12
    rel, dist = RP.intrinsics_error(torch.stack((K, _K(fy=190.0)))[None], torch.stack((K, K))[None])
    assert tuple(rel.shape) == (1, 2) and rel.dtype == torch.float64 and float(rel[0, 0]) == 0.0 and float(rel[0, 1]) == 0.5 and float(dist[0, 1]) == 0.0


def test_the_vertex_move_projects_where_the_stepped_K_would():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(8)
    d = torch.float64
    p = torch.from_numpy(rng.uniform(-2, 2, (1, 50, 3)) + [0.0, 0.0, 5.0])
    eye, zero = torch.eye(3, dtype=d)[None], torch.zeros(1, 1, 3, dtype=d)
    worst = 0.0
    for eps in (1e-9, 1e-2):
        for leaf in ([0.0, 0.0, 0.0, 0.0], [0.03, -0.02, 4.0, -6.5], [-0.3, 0.25, -40.0, 12.0]):
            K = _K()
            leaf = torch.tensor(leaf, dtype=d)
            moved = RP.intrinsics_move(p, leaf, float(K[0, 0]), float(K[1, 1]), proj_eps=eps)
            K2 = K.clone()
            K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2] = K[0, 0] * torch.exp(leaf[0]), K[1, 1] * torch.exp(leaf[1]), K[0, 2] + leaf[2], K[1, 2] + leaf[3]
            a = rr.project(moved, K[None], eye, zero, 512.0, eps=eps)
            b = rr.project(p, K2[None], eye, zero, 512.0, eps=eps)
            worst = max(worst, float((a - b).abs().max()))
            assert float((a - b).abs().max()) <= 1e-12
            if not leaf.any():
                assert torch.equal(moved, p)
    print("max |project(moved, K) - project(p, stepped K)| = %.3e" % worst)
    # and its gradient at 0 is (fx dL/dfx, fy dL/dfy, dL/dcx, dL/dcy)
    K = _K().requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((1, 50, 3)))
    (rr.project(p, K[None], eye, zero, 512.0) * w).sum().backward()
    leaf = torch.zeros(4, dtype=d, requires_grad=True)
    (rr.project(RP.intrinsics_move(p, leaf, 420.0, 380.0), _K()[None], eye, zero, 512.0) * w).sum().backward()
    want = torch.stack((420.0 * K.grad[0, 0], 380.0 * K.grad[1, 1], K.grad[0, 2], K.grad[1, 2]))
    assert float((leaf.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


def _views(R, V):
    RP = pkg("host.reproject")
    rng = np.random.default_rng(0)
    cams = [[RP.look_at_view(rng.uniform(0, 4, 3) + [0, 0, 5], rng.uniform(1, 3, 3))[:3] for _ in range(V)] for _ in range(R)]
    return tuple(torch.stack([torch.stack([cams[r][v][j] for v in range(V)]) for r in range(R)]) for j in range(3))


def test_check_intrinsics_accepts_and_normalises():
    RF = pkg("host.refine")
    views = RF.check_views(_views(2, 3), 2)
    assert RF.check_intrinsics(None, views, 2) is None and RF.check_intrinsics(None, None, 2) is None
    out = RF.check_intrinsics(dict(focal_step=1e-3, center_step=0), views, 2)
    assert out == dict(focal_step=1e-3, center_step=0.0, tie_focal=True, free=None, start=None)
    free = torch.tensor([[True, False, True], [False, False, True]])
    start = views[0].double() * torch.tensor([[1.03, 1.0, 1.0], [1.0, 1.03, 1.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    out = RF.check_intrinsics(dict(focal_step=0.0, center_step=2.0, tie_focal=False, free=free, start=start), views, 2)
    assert torch.equal(out["free"], free) and out["tie_focal"] is False
    assert out["start"].dtype == torch.float32 and tuple(out["start"].shape) == (2, 3, 3, 3) and torch.equal(out["start"], start.float())
    one = RF.check_views(tuple(x[0] for x in _views(2, 3)))
    out = RF.check_intrinsics(dict(focal_step=1.0, free=free[0], start=views[0][0]), one)
    assert tuple(out["free"].shape) == (1, 3) and tuple(out["start"].shape) == (1, 3, 3, 3)


def test_check_intrinsics_refuses():
    RF = pkg("host.refine")
    views = RF.check_views(_views(2, 3), 2)
    ok = dict(focal_step=1e-6, center_step=1e-3)
    with pytest.raises(ValueError, match="needs views"):
        RF.check_intrinsics(ok, None, 2)
    with pytest.raises(ValueError, match="dict"):
        RF.check_intrinsics((1e-6, 1e-3), views, 2)
    with pytest.raises(ValueError, match="unknown keys"):
        RF.check_intrinsics(dict(ok, step=1.0), views, 2)
    for key in ("focal_step", "center_step"):
        for bad in (-1e-3, float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ValueError, match=key):
                RF.check_intrinsics(dict(ok, **{key: bad}), views, 2)
    for bad in (1, 0.0, None, "yes"):
        with pytest.raises(ValueError, match="tie_focal"):
            RF.check_intrinsics(dict(ok, tie_focal=bad), views, 2)
    for bad in (torch.ones(2, 3, dtype=torch.uint8), torch.ones(2, 2, dtype=torch.bool), torch.ones(3, dtype=torch.bool), [[True] * 3] * 2,
                torch.ones(2, 3, 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match="free"):
            RF.check_intrinsics(dict(ok, free=bad), views, 2)
    K = views[0]
    for bad in ((K,), K[:, :2], K[0], K[..., :2], K.long(), K.half(), K.numpy(), (K, K)):
        with pytest.raises(ValueError, match="start"):
            RF.check_intrinsics(dict(ok, start=bad), views, 2)

    def changed(i, j, value):
        out = K.clone(); out[1, 2, i, j] = value
        return out

    for (i, j, value), what in (((0, 1, 1e-3), "skew"), ((1, 0, -2.0), "skew"), ((0, 0, 0.0), "not positive"), ((1, 1, -300.0), "not positive"),
                                ((2, 2, 1.001), "last row"), ((2, 0, 1e-6), "last row"), ((0, 2, float("nan")), "non-finite"),
                                ((1, 1, float("inf")), "non-finite")):
        with pytest.raises(ValueError, match=what):                    # the K the loop would start from
            RF.check_intrinsics(dict(ok, start=changed(i, j, value)), views, 2)
        if what != "non-finite":                                       # (check_views itself refuses a non-finite camera)
            with pytest.raises(ValueError, match=what):                # the K of the views themselves
                RF.check_intrinsics(ok, (changed(i, j, value), views[1], views[2]), 2)
    # the one-room form takes no room axis
    one = RF.check_views(tuple(x[0] for x in _views(2, 3)))
    with pytest.raises(ValueError, match="free"):
        RF.check_intrinsics(dict(ok, free=torch.ones(1, 3, dtype=torch.bool)), one)
    with pytest.raises(ValueError, match="start"):
        RF.check_intrinsics(dict(ok, start=K[:1]), one)
