"""Refinement of the camera poses of the target views, host side (DESIGN §4 "Camera poses of the target views"): the closed form of the pose
gradient against autograd, the float64 pose update and its helpers (``reproject.pose_step_torch``, ``rotation_exp``, ``pose_error``), what
``refine.check_poses`` refuses, and the float32 run of the restatement against the bound the kernel is held to.  No GPU: nothing here launches."""
import numpy as np
import pytest
import torch

from conftest import pkg

import pose_refine_cases as PC
import pose_refine_ref as PR

from oracle import raster_ref as rr


def _cases():
    return [(which, op) for which in ("three", "away") for op in PC.host_operands(which)]


def _autograd(op):
    """fp64 autograd through raster_ref.project on E (R p + t) + tau at omega = tau = 0: L = <faces of the view (fill_back copies included,
    culled faces zero), grad_faces> -> (d omega, d tau)"""
    RP = pkg("host.reproject")
    d = torch.float64
    p = torch.from_numpy(op["corners"]).to(d)
    K, Rm, t = (torch.from_numpy(op[k]).to(d) for k in ("K", "R", "t"))
    om, ta = torch.zeros(3, dtype=d, requires_grad=True), torch.zeros(3, dtype=d, requires_grad=True)
    W = RP._skew(om)
    E = torch.eye(3, dtype=d) + W + torch.matmul(W, W) / 2
    cam = torch.matmul(torch.matmul(p, Rm.t()) + t, E.t()) + ta
    faces = torch.from_numpy(op["faces"]).long()
    F = faces.shape[0]
    # the kernel's cull: the float32 camera z of the float32 operands
    kept = PR.pose_grad_ref(op["faces"], op["corners"], op["K"], op["R"], op["t"], op["grad_faces"], op["orig_size"], op["proj_eps"],
                           op["cull_eps"])[3]
    uvz = rr.project(cam[None], K[None], torch.eye(3, dtype=d)[None], torch.zeros(1, 1, 3, dtype=d), op["orig_size"], eps=op["proj_eps"])
    f = rr.vertices_to_faces(uvz, faces[None])[0]
    f = torch.where(torch.from_numpy(kept)[:, None, None], f, torch.zeros_like(f))
    w = torch.from_numpy(op["grad_faces"]).to(d)
    (torch.cat((f, f[:, [2, 1, 0]])) * w[:2 * F]).sum().backward()
    return torch.cat((om.grad, ta.grad)).numpy()


def test_closed_form_is_the_autograd_gradient_in_fp64():
    seen = 0
    for which, op in _cases():
        g, S, n, kept = PR.pose_grad_ref(*(op[k] for k in ("faces", "corners", "K", "R", "t", "grad_faces", "orig_size", "proj_eps", "cull_eps")))
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


def test_the_cases_cull_what_they_say():
    for which, op in _cases():
        kept = PR.pose_grad_ref(*(op[k] for k in ("faces", "corners", "K", "R", "t", "grad_faces", "orig_size", "proj_eps", "cull_eps")))[3]
        if which == "away" and op["v"] == 0:
            assert not kept.any(), "the view that looks away keeps a face"
        elif op["v"] == 1:
            assert kept.all(), "the outside view culls a face"
        elif which == "three" and op["v"] == 2:
            assert 0 < int(kept.sum()) < kept.size, "the view from inside object 0 does not cull PART of the room"


def test_float32_restatement_stays_within_half_the_kernels_bound():
    """the kernel is held to (POSE_C + 0.5 sqrt(n)) 2^-24 S; a float32 run of the restatement (products in float32 in the kernel's order, sums in
    float64) must lie within HALF of it for every case of tests/test_place_pose_gpu.py.  Measured here (LAB_NOTES "Camera poses of the target
    views"): worst ratio 0.0030 of the bound - the constant 36 stays."""
    worst = 0.0
    for which, op in _cases():
        args = tuple(op[k] for k in ("faces", "corners", "K", "R", "t", "grad_faces", "orig_size", "proj_eps", "cull_eps"))
        g64, S, n, _ = PR.pose_grad_ref(*args)
        g32 = PR.pose_grad_ref(*args, dtype=np.float32)[0]
        if n == 0:
            assert not g32.any()
            continue
        ratio = np.abs(g32 - g64) / PR.pose_bound(S, n)
        print("%s room %d view %d: n = %d, |float32 - float64| / bound per element: %s" % (which, op["r"], op["v"], n, np.array2string(ratio, precision=4)))
        worst = max(worst, float(ratio.max()))
    print("worst ratio %.4f" % worst)
    assert 0 < worst <= 0.5


def test_pose_step_keeps_a_rotation_a_rotation():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(3)
    _, R0, t, _ = RP.look_at_view([5.0, 3.0, 7.0], [2.0, 1.0, 2.0])
    # (look_at_view rounds its rotation to float32, orthonormal to 1e-7 only: the 64 steps start from the nearest float64 rotation)
    U, _, Vh = torch.linalg.svd(R0.double())
    Rm = U @ Vh
    for _ in range(64):
        w = rng.standard_normal(3); w *= rng.uniform(0, 0.05) / np.linalg.norm(w)
        Rm, t = RP.pose_step_torch(Rm, t, torch.from_numpy(w), torch.from_numpy(rng.uniform(-0.05, 0.05, 3)))
    off = float((Rm @ Rm.t() - torch.eye(3, dtype=torch.float64)).abs().max())
    print("|R R^T - I| after 64 steps: %.3e, det %.17g" % (off, float(torch.linalg.det(Rm))))
    assert Rm.dtype == torch.float64 and t.dtype == torch.float64
    assert off <= 1e-12 and abs(float(torch.linalg.det(Rm)) - 1.0) <= 1e-12


def test_pose_step_with_zero_rotation_is_a_pure_translation_by_bits():
    RP = pkg("host.reproject")
    _, Rm, t, _ = RP.look_at_view([5.0, 3.0, 7.0], [2.0, 1.0, 2.0])
    tau = torch.tensor([0.3, -0.7, 1e-9], dtype=torch.float64)
    R1, t1 = RP.pose_step_torch(Rm, t, torch.zeros(3), tau)
    assert torch.equal(R1.view(torch.int64), Rm.double().view(torch.int64))
    assert torch.equal(t1.view(torch.int64), (t.double() + tau).view(torch.int64))
    # batched, and the master of a float32 table entry is exactly its double
    R2, t2 = RP.pose_step_torch(torch.stack((Rm, Rm)), torch.stack((t, t)), torch.zeros(2, 3), torch.stack((tau, 2 * tau)))
    assert torch.equal(R2[1], Rm.double()) and torch.equal(t2[1], t.double() + 2 * tau)


def test_series_and_rodrigues_agree_at_the_switch():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(9)
    for _ in range(16):
        w = rng.standard_normal(3); w *= RP.SMALL_ANGLE / np.linalg.norm(w)
        a, b = RP.rotation_exp(torch.from_numpy(w), series=True), RP.rotation_exp(torch.from_numpy(w), series=False)
        assert float((a - b).abs().max()) <= 1e-15
    big = torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)
    assert float((RP.rotation_exp(big) - torch.linalg.matrix_exp(RP._skew(big))).abs().max()) <= 1e-15
    assert torch.equal(RP.rotation_exp(torch.zeros(3)), torch.eye(3, dtype=torch.float64))


def test_pose_error_of_a_pose_with_itself_is_zero_and_measures_what_it_says():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(4)
    for _ in range(8):
        _, Rm, t, _ = RP.look_at_view(rng.uniform(3, 6, 3), rng.uniform(0, 2, 3))
        ang, dist = RP.pose_error(Rm, t, Rm, t)
        assert float(ang) == 0.0 and float(dist) == 0.0
        w = torch.from_numpy(rng.standard_normal(3)); w = w * 0.02 / w.norm()
        R1, t1 = RP.pose_step_torch(Rm, t, w, torch.zeros(3))
        ang, dist = RP.pose_error(R1, t1, Rm, t)
        # (a rotation of the camera frame about its origin keeps the centre -R^T E^T E t; Rm is a float32 rotation, orthonormal to 1e-7)
        assert abs(float(ang) - 0.02) <= 1e-7 and float(dist) <= 1e-7
        R2, t2 = RP.pose_step_torch(Rm, t, torch.zeros(3), torch.tensor([0.0, 0.02, 0.0]))
        ang, dist = RP.pose_error(R2, t2, Rm, t)
        assert float(ang) == 0.0 and abs(float(dist) - 0.02) <= 1e-7
    ang, dist = RP.pose_error(torch.stack((Rm.double(), R1)), torch.stack((t.double(), t1)), torch.stack((Rm, Rm)), torch.stack((t, t)))
    assert tuple(ang.shape) == (2,) and float(ang[0]) == 0.0 and float(ang[1]) > 0


def _views(R, V):
    RP = pkg("host.reproject")
    rng = np.random.default_rng(0)
    cams = [[RP.look_at_view(rng.uniform(0, 4, 3) + [0, 0, 5], rng.uniform(1, 3, 3))[:3] for _ in range(V)] for _ in range(R)]
    return tuple(torch.stack([torch.stack([cams[r][v][j] for v in range(V)]) for r in range(R)]) for j in range(3))


def test_check_poses_accepts_and_normalises():
    RF = pkg("host.refine")
    views = RF.check_views(_views(2, 3), 2)
    assert RF.check_poses(None, views, 2) is None and RF.check_poses(None, None, 2) is None
    out = RF.check_poses(dict(rot_step=1e-3, trans_step=0), views, 2)
    assert out == dict(rot_step=1e-3, trans_step=0.0, free=None, start=None)
    free = torch.tensor([[True, False, True], [False, False, True]])
    start = (views[1].double(), views[2].double())
    out = RF.check_poses(dict(rot_step=0.0, trans_step=2.0, free=free, start=start), views, 2)
    assert torch.equal(out["free"], free) and out["start"][0].dtype == torch.float32 and torch.equal(out["start"][0], views[1])
    assert torch.equal(out["start"][1], views[2])
    one = RF.check_views(tuple(x[0] for x in _views(2, 3)))
    out = RF.check_poses(dict(rot_step=1.0, free=free[0], start=(views[1][0], views[2][0])), one)
    assert tuple(out["free"].shape) == (1, 3) and tuple(out["start"][0].shape) == (1, 3, 3, 3) and tuple(out["start"][1].shape) == (1, 3, 3)


def test_check_poses_refuses():
    RF = pkg("host.refine")
    views = RF.check_views(_views(2, 3), 2)
    ok = dict(rot_step=1e-3, trans_step=1e-3)
    with pytest.raises(ValueError, match="needs views"):
        RF.check_poses(ok, None, 2)
    with pytest.raises(ValueError, match="dict"):
        RF.check_poses((1e-3, 1e-3), views, 2)
    with pytest.raises(ValueError, match="unknown keys"):
        RF.check_poses(dict(ok, step=1.0), views, 2)
    for key in ("rot_step", "trans_step"):
        for bad in (-1e-3, float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ValueError, match=key):
                RF.check_poses(dict(ok, **{key: bad}), views, 2)
    for bad in (torch.ones(2, 3, dtype=torch.uint8), torch.ones(2, 2, dtype=torch.bool), torch.ones(3, dtype=torch.bool), [[True] * 3] * 2,
                torch.ones(2, 3, 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match="free"):
            RF.check_poses(dict(ok, free=bad), views, 2)
    Rm, t = views[1], views[2]
    for bad in ((Rm,), (Rm, t, t), (Rm[:, :2], t[:, :2]), (Rm, t[..., :2]), (Rm[0], t[0]), (Rm.long(), t), (Rm, t.half()), (Rm.numpy(), t.numpy()), Rm):
        with pytest.raises(ValueError, match="start"):
            RF.check_poses(dict(ok, start=bad), views, 2)
    skew = Rm.clone(); skew[1, 2, 0, 0] += 3e-4
    with pytest.raises(ValueError, match="orthonormal"):
        RF.check_poses(dict(ok, start=(skew, t)), views, 2)
    nan = t.clone(); nan[0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        RF.check_poses(dict(ok, start=(Rm, nan)), views, 2)
    almost = Rm.clone(); almost[1, 2, 0, 0] += 1e-5                       # inside the tolerance: float32 cameras are not exact rotations
    assert RF.check_poses(dict(ok, start=(almost, t)), views, 2) is not None
    # the one-room form takes no room axis
    one = RF.check_views(tuple(x[0] for x in _views(2, 3)))
    with pytest.raises(ValueError, match="free"):
        RF.check_poses(dict(ok, free=torch.ones(1, 3, dtype=torch.bool)), one)
    with pytest.raises(ValueError, match="start"):
        RF.check_poses(dict(ok, start=(Rm[:1], t[:1])), one)
