"""Several target views per room, host side (DESIGN §4 "Several target views per room"): the cameras ``reproject.look_at_view`` builds
and what ``refine.check_views`` refuses.  No GPU: nothing here launches."""
import numpy as np
import pytest
import torch

from conftest import pkg

ROOMS = ([0, 0, 0, 4.0, 2.7, 5.0], [0, 0, 0, 3.6, 2.4, 4.4], [0, 0, 0, 5.5, 0.15, 6.0])       # (the last: min(0.1, |h / 2|) takes |h / 2|)


def _cam_eye(room):
    return np.array([room[3] / 2.0, room[4] / 2.0 + min(0.1, abs(room[4] / 2.0)), room[5]], np.float64)


@pytest.mark.parametrize("room", ROOMS)
def test_look_at_view_from_the_refinement_eye_along_its_axis_is_get_cam_mat(room):
    RP, DR = pkg("host.reproject"), pkg("host.diff_render")
    K0, R0, t0 = DR.get_cam_mat([room], "cpu")
    eye = _cam_eye(room)
    axis = np.array([0.0, np.sin(-0.4), -np.cos(-0.4)])                  # the camera looks along -z of w2c: minus its third row
    for dist in (0.5, 3.0):
        K, R, t, orig = RP.look_at_view(eye, eye + dist * axis)
        assert K.dtype == R.dtype == t.dtype == torch.float32 and K.shape == (3, 3) and R.shape == (3, 3) and t.shape == (3,)
        assert orig == float(DR.inter_out) and torch.equal(K, K0[0])
        assert float((R - R0[0]).abs().max()) <= 1e-6, (R, R0)
        assert float((t - t0.reshape(3)).abs().max()) <= 1e-6, (t, t0)
        Kr, Rr, tr, _ = RP.refine_view(room, 64)
        assert torch.equal(K, Kr) and float((R - Rr).abs().max()) <= 1e-6 and float((t - tr).abs().max()) <= 1e-6


def test_look_at_view_is_a_proper_rotation_without_roll():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(5)
    for _ in range(20):
        eye, at = rng.uniform(-3, 6, 3), rng.uniform(-3, 6, 3)
        _, R, t, _ = RP.look_at_view(eye, at)
        R64 = R.double().numpy()
        assert np.abs(R64 @ R64.T - np.eye(3)).max() <= 1e-6
        assert abs(np.linalg.det(R64) - 1.0) <= 1e-6
        # the eye is the camera's origin, the looked-at point lies on the +z axis (c2cv: the camera looks along +z), the world's
        # y axis has no x component in the image (no roll) and points up (-y after the flip)
        assert np.abs(R64 @ eye + t.double().numpy()).max() <= 1e-5
        p = R64 @ at + t.double().numpy()
        assert abs(p[0]) <= 1e-5 and abs(p[1]) <= 1e-5 and abs(p[2] - np.linalg.norm(at - eye)) <= 1e-5
        assert abs(R64[0, 1]) <= 1e-6 and R64[1, 1] < 0
    for bad in (([0, 1, 0], [0, 1, 0]), ([1, 0, 1], [1, 5, 1]), ([0, float("nan"), 0], [1, 1, 1]), ([0, 0], [1, 1, 1])):
        with pytest.raises(ValueError, match="look_at_view"):
            RP.look_at_view(*bad)


def _views(R, V, seed=0):
    RP = pkg("host.reproject")
    rng = np.random.default_rng(seed)
    cams = [[RP.look_at_view(rng.uniform(0, 4, 3) + [0, 0, 5], rng.uniform(1, 3, 3))[:3] for _ in range(V)] for _ in range(R)]
    return tuple(torch.stack([torch.stack([cams[r][v][j] for v in range(V)]) for r in range(R)]) for j in range(3))


def test_check_views_accepts_and_normalises():
    RF = pkg("host.refine")
    assert RF.check_views(None, 2) is None and RF.check_views(None) is None
    K, Rm, t = _views(2, 3)
    out = RF.check_views((K, Rm, t), 2)
    assert [tuple(x.shape) for x in out] == [(2, 3, 3, 3), (2, 3, 3, 3), (2, 3, 3)]
    assert all(x.dtype == torch.float32 and x.device.type == "cpu" and x.is_contiguous() for x in out)
    assert all(torch.equal(a, b) for a, b in zip(out, (K, Rm, t)))
    # numpy / float64 / lists come out the same; the one-room form gains the room axis
    out64 = RF.check_views([K.double().numpy(), Rm.tolist(), t.double()], 2)
    assert all(torch.equal(a, b) for a, b in zip(out, out64))
    one = RF.check_views((K[0], Rm[0], t[0]))
    assert [tuple(x.shape) for x in one] == [(1, 3, 3, 3), (1, 3, 3, 3), (1, 3, 3)] and torch.equal(one[0][0], K[0])
    # V = 64 is the most; observed / mask with the V axis pass
    big = _views(1, 64)
    assert RF.check_views(big, 1)[0].shape[1] == 64
    S = 8
    obs = (torch.zeros(2, 3, S, S), torch.zeros(2, 3, S, S, dtype=torch.uint8))
    assert RF.check_views((K, Rm, t), 2, observed=obs, mask=torch.ones(2, 3, S, S, dtype=torch.uint8)) is not None
    assert RF.check_views((K, Rm, t), 2, observed=obs, mask="readings") is not None
    assert RF.check_views((K[0], Rm[0], t[0]), None, mask=torch.ones(3, S, S, dtype=torch.bool)) is not None


def test_check_views_refuses():
    RF = pkg("host.refine")
    K, Rm, t = _views(2, 3)
    S = 8
    shapes = [(K, Rm), (K, Rm, t, t), (K[0], Rm[0], t[0]), (K, Rm, t[:, :2]), (K, Rm[:, :, :2], t), (K[:, :, :, :2], Rm, t), (K, Rm, t[..., None]),
              (K[:, :0], Rm[:, :0], t[:, :0]), (K[:1], Rm[:1], t[:1]), K]
    for bad in shapes:
        with pytest.raises(ValueError, match="views"):
            RF.check_views(bad, 2)
    with pytest.raises(ValueError, match="views"):
        RF.check_views((K, Rm, t))                                        # the one-room form takes no room axis
    with pytest.raises(ValueError, match="views"):
        RF.check_views(("a", "b", "c"), 2)
    with pytest.raises(ValueError, match="at most 64"):
        RF.check_views(_views(1, 65), 1)
    for j, val in ((0, float("nan")), (1, float("inf")), (2, float("-inf"))):
        bad = [K.clone(), Rm.clone(), t.clone()]
        bad[j].view(-1)[5] = val
        with pytest.raises(ValueError, match="non-finite"):
            RF.check_views(tuple(bad), 2)
    # observed / mask without the V axis
    with pytest.raises(ValueError, match="V axis"):
        RF.check_views((K, Rm, t), 2, observed=(torch.zeros(2, S, S), torch.zeros(2, S, S, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="V axis"):
        RF.check_views((K, Rm, t), 2, mask=torch.ones(2, S, S, dtype=torch.uint8))
    with pytest.raises(ValueError, match="V axis"):
        RF.check_views((K, Rm, t), 2, mask=torch.ones(2, 2, S, S, dtype=torch.uint8))
    with pytest.raises(ValueError, match="V axis"):
        RF.check_views((K[0], Rm[0], t[0]), None, mask=torch.ones(S, S, dtype=torch.uint8))
    # out of scope together with views
    for kw in (dict(report="ends"), dict(pictures="all"), dict(retrieve=True)):
        with pytest.raises(ValueError, match="does not combine"):
            RF.check_views((K, Rm, t), 2, **kw)
