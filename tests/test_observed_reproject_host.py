"""Reprojection of observed frames, host side (host/reproject.py; CPU-only): the torch definition against closed forms and brute force,
the conditions the shared cases must meet, the camera helpers, the argument checks of the two entry points (which run before anything is
launched, so they need no device) and the measured figures the GPU tests' allowances are multiples of."""
import ctypes as C

import numpy as np
import pytest
import torch

import observed_reproject_cases as OC
from conftest import load_golden, pkg

CASES = OC.cases()


def _kept(f):
    return ~(f == 0).all(-1).all(-1)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.NAMES)
def test_every_case_meets_the_two_conditions(name):
    """float32 and float64 collapse the same slots (steps stay outside [gap / 2, 2 gap] of the nearer depth, z stays 1e-3 away from
    near), and a frame meant to show a surface hits a quarter of the target under the float64 route"""
    RP = pkg("host.reproject")
    c = OC.case(name)
    w64, w32 = OC.torch_route(c, torch.float64), OC.torch_route(c, torch.float32)
    assert OC.face_error(w32["faces_xyz"], w64["faces_xyz"])[1] == 0
    d = c["depth_src"]
    B, Hs, Ws = d.shape
    assert w64["faces_xyz"].shape == (B, 2 * (Hs - 1) * (Ws - 1), 3, 3) and w64["depth"].shape == (B, c["S"], c["S"])
    reading = (d > 0) & (d <= 15)
    a, b, cc, dd = d[:, :-1, :-1], d[:, 1:, :-1], d[:, :-1, 1:], d[:, 1:, 1:]
    ra, rb, rc, rd = reading[:, :-1, :-1], reading[:, 1:, :-1], reading[:, :-1, 1:], reading[:, 1:, 1:]
    for (p, q, r), ok in (((a, b, cc), ra & rb & rc), ((dd, cc, b), rd & rc & rb)):
        lo, hi = torch.minimum(p, torch.minimum(q, r)).double(), torch.maximum(p, torch.maximum(q, r)).double()
        rel = ((hi - lo) / lo)[ok]
        assert not bool(((rel >= 0.5 * c["gap"]) & (rel <= 2.0 * c["gap"])).any()), "a step inside [gap / 2, 2 gap]"
    # every vertex with a reading, whatever the other rules do with its slots: z stays away from near
    free = RP.faces_torch(d, c["k_src"], c["pose"], c["K_tgt"], c["orig_size"], near=1e-30, gap=1e30, dtype=torch.float64)
    live = _kept(free)
    z = free[..., 2][live]
    if z.numel():
        assert float((z - c["near"]).abs().min()) >= 1e-3
    for b_, shows in enumerate(c["shows"]):
        hits = int(w64["hits"][b_])
        assert hits == int((w64["depth"][b_] > 0).sum()) == int(w32["hits"][b_])
        if shows is True:
            assert 4 * hits >= c["S"] ** 2, "frame %d hits %d of %d" % (b_, hits, c["S"] ** 2)
        if shows is False:
            assert hits == 0 and bool((w64["depth"][b_] == -1).all()) and bool((w64["labels"][b_] == 0).all())


def test_the_cases_hold_what_they_are_there_for():
    t = OC.case("tile_edge_18x34_s32")
    w = OC.torch_route(t, torch.float64)
    kept = _kept(w["faces_xyz"]).reshape(3, 17, 33, 2)
    # frame 1: the step of 2 against 3 between columns 19 and 20 cuts, the step of 2 against 2.02 between rows 9 and 10 does not
    assert not bool(kept[1, :, 19].any()) and bool(kept[1, :, :19].all()) and bool(kept[1, :, 20:].all()) and bool(kept[1, 9, :19].all())
    # frame 2: exactly the slots that touch one of the seven pixels without a reading are gone
    bad = ~((t["depth_src"][2] > 0) & (t["depth_src"][2] <= 15))
    assert int(bad.sum()) == 7
    a, b, c, d = bad[:-1, :-1], bad[1:, :-1], bad[:-1, 1:], bad[1:, 1:]
    assert torch.equal(~kept[2, :, :, 0], a | b | c) and torch.equal(~kept[2, :, :, 1], d | c | b)
    assert {0, 41, 255} <= set(w["labels"][2].flatten().tolist()), "the bytes 0, 41 and 255 pass through"
    f = OC.case("frames_48x64_s64")
    w = OC.torch_route(f, torch.float64)
    kept = _kept(w["faces_xyz"])
    # seen from behind: every slot is kept and in front of the camera - the rasterizer's back-face test alone drops the surface
    assert bool(kept[1].all()) and float(w["faces_xyz"][1, :, :, 2].min()) > 1.0 and int(w["hits"][1]) == 0
    # corners inside near: the slots of the patch and of its rim collapse by that rule alone (14 x 13 pixels: 15 x 14 cells), the rest stay
    assert int((~kept[2]).sum()) == 2 * 15 * 14 - 2 and int(w["hits"][2]) > 0
    n = OC.case("nothing_to_show_3x5_s16")
    w = OC.torch_route(n, torch.float64)
    assert _kept(w["faces_xyz"]).sum(1).tolist() == [0, 0, 16]
    assert bool(((n["depth_src"][1] > 0) & (n["depth_src"][1] <= 15)).all()), "the frame with fx = 0 is a sound frame otherwise"


# ------------------------------------------------------------------------------------------------------------------------------
# the definition against closed forms and brute force
# ------------------------------------------------------------------------------------------------------------------------------
def _loop_faces(depth, k, P, K, os_, near, gap):
    """the definition once more, slot by slot in Python floats (float64; the two float32 decisions in numpy float32)"""
    Hs, Ws = depth.shape
    out = np.zeros((2 * (Hs - 1) * (Ws - 1), 3, 3))

    def vertex(i, j):
        d = float(depth[i, j])
        xs, ys = (j + 0.5 - k[2]) / k[0] * d, (i + 0.5 - k[3]) / k[1] * d
        x, y, z = (P[r, 0] * xs + P[r, 1] * ys + P[r, 2] * d + P[r, 3] for r in range(3))
        xh, yh = x / (z + 1e-9), y / (z + 1e-9)
        u, v = K[0, 0] * xh + K[0, 1] * yh + K[0, 2], os_ - (K[1, 0] * xh + K[1, 1] * yh + K[1, 2])
        return (2 * (u - os_ / 2) / os_, 2 * (v - os_ / 2) / os_, z)
    for i in range(Hs - 1):
        for j in range(Ws - 1):
            a, b, c, d = (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1)
            for which, tri in enumerate(((a, b, c), (d, c, b))):
                ds = [np.float32(depth[p]) for p in tri]
                if not all(bool(x > 0) and bool(x <= 15) for x in ds):
                    continue
                if np.float32(max(ds)) - np.float32(min(ds)) > np.float32(gap) * np.float32(min(ds)):
                    continue
                vs = [vertex(*p) for p in tri]
                if not all(v[2] >= near for v in vs) or not (k[0] > 0 and k[1] > 0):
                    continue
                out[2 * (i * (Ws - 1) + j) + which] = vs
    return out


@pytest.mark.parametrize("rule", ["none", "reading", "step", "near", "focal"])
def test_collapse_rules_one_at_a_time(rule):
    """a 4 x 5 frame of a sound surface; one rule at a time is made to bite, and the slots that go are exactly the loop restatement's"""
    RP = pkg("host.reproject")
    Hs, Ws = 4, 5
    k = OC._k_src(Hs, Ws)
    depth = OC._plane_depth(Hs, Ws, k, *OC.GENTLE).astype(np.float32)
    P, K, near = OC._pose(0.03, -0.05, (0.1, 0.0, 0.2)), OC._k_tgt(300.0), 0.1
    gone = None
    if rule == "reading":
        depth[1, 2] = np.nan; depth[3, 0] = 15.5; depth[0, 4] = 0.0
        gone = 6 + 2 + 2                                             # an inner pixel touches six slots, a b or c corner of the grid two
    if rule == "step":
        depth[:, 3:] *= np.float32(1.2)
        gone = 2 * (Hs - 1)                                          # the column of cells across the step
    if rule == "near":
        P = OC._pose(0.0, 0.0, (0.0, 0.0, -2.40))                    # the surface's near part comes to rest inside near
    if rule == "focal":
        k = k.copy(); k[1] = 0.0
    args = [torch.from_numpy(np.asarray(x, np.float64)[None].astype(np.float32)) for x in (depth, k, P, K)]
    got = RP.faces_torch(*args, OC.ORIG, near=near, gap=OC.GAP, dtype=torch.float64)[0]
    with np.errstate(all="ignore"):                                  # (the frame with fy = 0 divides by it, as the routes do)
        want = _loop_faces(depth, *(a[0].double().numpy() for a in args[1:]), OC.ORIG, near, OC.GAP)
    kept_g, kept_w = _kept(got), _kept(torch.from_numpy(want))
    assert torch.equal(kept_g, kept_w)
    assert float((got - torch.from_numpy(want)).abs().max()) <= 1e-12
    F = 2 * (Hs - 1) * (Ws - 1)
    if rule == "none":
        assert int(kept_g.sum()) == F
    elif rule == "focal":
        assert int(kept_g.sum()) == 0
    elif rule == "near":
        assert 0 < int(kept_g.sum()) < F
        z = RP.faces_torch(*args, OC.ORIG, near=1e-30, gap=OC.GAP, dtype=torch.float64)[0][..., 2]
        assert torch.equal(kept_g, (z >= near).all(-1)) and float((z - near).abs().min()) > 1e-4       # (two float64 routes: far enough)
    else:
        assert int((~kept_g).sum()) == gone


def _plane_frames():
    return [(c, b) for c in CASES for b in range(len(c["plane"])) if c["plane"][b] is not None and c["shows"][b] is not False]


def test_planes_against_the_closed_form_ray_plane_depth():
    """float64 route: perspective-correct interpolation is exact on a plane, so what is left is the float32 rasterizer's rounding - held
    to the bound observed_reproject_cases.raster_bound derives from its arithmetic.  Every pixel whose source position lies a full source
    pixel inside the grid is hit wherever the frame has no hole."""
    checked = 0
    for c, b in _plane_frames():
        want, inside, _, _ = OC.closed_form(c, b)
        w = OC.torch_route(c, torch.float64)
        hit = w["depth"][b] > 0
        if bool(_kept(w["faces_xyz"][b]).all()):
            assert not bool((inside & ~hit).any()), (c["name"], b)
        m = inside & hit
        if not bool(m.any()):
            continue
        err, bound = float((w["depth"][b].double() - want)[m].abs().max()), OC.raster_bound(c, w["faces_xyz"], b)
        print("%s frame %d: float64 route against the closed form on %d pixels: %.3e (bound %.3e)" % (c["name"], b, int(m.sum()), err, bound))
        assert err <= bound
        checked += int(m.sum())
    assert checked > 5000


def test_label_is_the_nearest_source_pixels_where_a_weight_exceeds_one_half():
    """The corner of largest weight is the nearest source pixel wherever that weight exceeds 1/2 (between, the rule picks a corner of the
    face: at most one pixel away).  Brute force: the source position of a target pixel from the closed form, the nearest pixel centre, and
    the barycentric weights of the position in its cell's triangle - compared where the largest exceeds 0.6, away from the ties."""
    checked = 0
    for c, b in _plane_frames():
        _, inside, us, vs = OC.closed_form(c, b)
        w = OC.torch_route(c, torch.float64)
        hit = w["depth"][b] > 0
        x, y = (us - 0.5) - torch.floor(us - 0.5), (vs - 0.5) - torch.floor(vs - 0.5)
        upper = x + y < 1                                            # slot (a, b, c); else (d, c, b)
        top = torch.where(upper, torch.maximum(1 - x - y, torch.maximum(x, y)), torch.maximum(x + y - 1, torch.maximum(1 - x, 1 - y)))
        m = inside & hit & (top > 0.6)
        near_lab = c["labels_src"][b][torch.floor(vs).long().clamp(0, c["labels_src"].shape[1] - 1), torch.floor(us).long().clamp(0, c["labels_src"].shape[2] - 1)]
        assert torch.equal(w["labels"][b][m], near_lab[m]), (c["name"], b)
        checked += int(m.sum())
        assert len(set(near_lab[m].tolist())) > 3 or int(m.sum()) < 50
    assert checked > 2000


def test_compose_on_hand_made_maps_in_torch():
    RP = pkg("host.reproject")
    Hs, Ws, S = 3, 4, 3
    lab = torch.arange(1, 13, dtype=torch.uint8).reshape(1, Hs, Ws)
    F = RP.n_faces(Hs, Ws)
    fi = torch.tensor([[[-1, F, F + 1000], [0, 1, 7], [2, 3, 11]]], dtype=torch.int32)
    w = torch.tensor([0.2, 0.3, 0.5]).repeat(1, S, S, 1).clone()
    w[0, 1, 0] = torch.tensor([0.4, 0.4, 0.2])                       # a tie of two: the lower corner number
    w[0, 1, 1] = torch.tensor([1 / 3, 1 / 3, 1 / 3])                 # a tie of three
    w[0, 1, 2] = torch.tensor([0.1, float("nan"), 0.9])              # a NaN: no hit
    dep = torch.arange(9, dtype=torch.float32).reshape(1, S, S) + 1
    d, l, hits = RP.compose_torch(fi, w, dep, lab)
    # raster row 0 is the planes' last row.  Raster row 1: slot 0 = (a, b, c) of cell (0, 0), corner 0 = a = pixel (0, 0) -> 1; slot 1 =
    # (d, c, b) of that cell, corner 0 = d = pixel (1, 1) -> 6; the NaN.  Raster row 2, corner 2 everywhere: slot 2 of cell (0, 1): c =
    # pixel (0, 2) -> 3; slot 3 of it: b = pixel (1, 1) -> 6; slot 11 = (d, c, b) of cell (1, 2): b = pixel (2, 2) -> 11
    assert l[0].tolist() == [[3, 6, 11], [1, 6, 0], [0, 0, 0]]
    assert d[0].tolist() == [[7.0, 8.0, 9.0], [4.0, 5.0, -1.0], [-1.0, -1.0, -1.0]] and hits.tolist() == [5]


# ------------------------------------------------------------------------------------------------------------------------------
# helpers and checks
# ------------------------------------------------------------------------------------------------------------------------------
def test_relative_pose_takes_source_coordinates_to_target_coordinates():
    RP = pkg("host.reproject")
    rng = np.random.default_rng(4)
    Rs, Rt = OC._rot(0.3, -0.7), OC._rot(-0.2, 1.1)
    ts, tt = rng.normal(size=3), rng.normal(size=3)
    pose = RP.relative_pose(torch.from_numpy(Rs)[None], torch.from_numpy(ts)[None, None], torch.from_numpy(Rt)[None], torch.from_numpy(tt)[None])
    assert pose.shape == (1, 3, 4) and pose.dtype == torch.float32
    want = np.concatenate([Rt @ Rs.T, (tt - Rt @ Rs.T @ ts)[:, None]], 1)
    assert torch.equal(pose[0], torch.from_numpy(want).float()), "float64 arithmetic, rounded once"
    world = rng.normal(size=(20, 3))
    ps, pt = world @ Rs.T + ts, world @ Rt.T + tt
    assert np.abs(ps @ want[:, :3].T + want[:, 3] - pt).max() < 1e-12
    same = RP.relative_pose(Rs, ts, Rs, ts)
    assert np.abs(same.numpy() - np.eye(3, 4)).max() < 1e-7


def test_scene_as_source_and_refine_view():
    """under scene_as_source and the identity pose, vertex (i, j) of the mesh is the centre of the plane pixel (i, j): raster pixel
    (S - 1 - i, j).  No axis is mirrored."""
    RP, DR = pkg("host.reproject"), pkg("host.diff_render")
    room = [0.0, 0.0, 0.0, 3.7, 2.7, 4.5]
    S = 8
    K, R, t, orig = RP.refine_view(room, S)
    Kw, Rw, tw = DR.get_cam_mat([room], "cpu")
    assert torch.equal(K, Kw[0]) and torch.equal(R, Rw[0]) and torch.equal(t, tw.reshape(3)) and orig == 512.0
    k = RP.scene_as_source(K, orig, S)
    assert k.tolist() == [200.0 * S / 512, 200.0 * S / 512, S / 2, S / 2] and k.dtype == torch.float32
    assert RP.scene_as_source(K[None], orig, S).shape == (1, 4)
    k_src, pose, K_tgt, orig = OC.round_trip_inputs(room, S)
    depth = torch.full((1, S, S), 2.0)
    f = RP.faces_torch(depth, k_src, pose, K_tgt, orig, dtype=torch.float64).reshape(S - 1, S - 1, 2, 3, 3)
    i, j = torch.meshgrid(torch.arange(S - 1), torch.arange(S - 1), indexing="ij")
    a = f[:, :, 0, 0]                                                 # corner a of slot 0 is pixel (i, j)
    assert float((a[..., 0] - (2.0 * j + 1 - S) / S).abs().max()) < 1e-9
    assert float((a[..., 1] + (2.0 * i + 1 - S) / S).abs().max()) < 1e-9 and bool((a[..., 2] == 2.0).all())
    d = f[:, :, 1, 0]                                                 # corner d of slot 1 is pixel (i + 1, j + 1)
    assert float((d[..., 0] - (2.0 * (j + 1) + 1 - S) / S).abs().max()) < 1e-9 and float((d[..., 1] + (2.0 * (i + 1) + 1 - S) / S).abs().max()) < 1e-9


def test_argument_checks_refuse_before_any_launch():
    """host tensors stand in for the device buffers: every call below returns before a launch, none of the buffers is read"""
    RP, L = pkg("host.reproject"), pkg("_lib")
    lib = L.lib()
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    dep, k, P, K, fx = f32(1, 3, 4), f32(1, 4), f32(1, 3, 4), f32(1, 3, 3), f32(1, 12, 3, 3)

    def faces(B=1, Hs=3, Ws=4, orig=512.0, near=0.1, gap=0.05, out=fx, **null):
        d = L.SlnReproject()
        d.depth_src, d.k_src, d.pose, d.K_tgt = (None if n in null else t.data_ptr() for n, t in (("depth_src", dep), ("k_src", k), ("pose", P), ("K_tgt", K)))
        d.B, d.Hs, d.Ws, d.orig_size, d.near, d.gap = B, Hs, Ws, orig, near, gap
        return lib.sln_reproject_faces(d, None if out is None else C.c_void_p(out.data_ptr() if torch.is_tensor(out) else out), None)
    nan = float("nan")
    for kw in (dict(B=0), dict(B=65536), dict(Hs=1), dict(Ws=1), dict(Hs=4097, Ws=2050), dict(orig=0.0), dict(orig=-512.0), dict(orig=nan),
               dict(near=0.0), dict(near=-0.1), dict(near=nan), dict(gap=-0.01), dict(gap=nan), dict(out=None), dict(out=fx.data_ptr() + 4),
               dict(depth_src=1), dict(k_src=1), dict(pose=1), dict(K_tgt=1)):
        assert faces(**kw) == -1, kw
    assert lib.sln_reproject_faces(None, C.c_void_p(fx.data_ptr()), None) == -1
    assert 2 * 4096 * 2049 > 2 ** 24 >= 2 * 4096 * 2048
    with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
        RP.faces(dep, k, P, K, 512.0, 0.0, 0.05, fx)

    S = 8
    fi, w, rd = torch.zeros(1, S, S, dtype=torch.int32), f32(1, S, S, 3), f32(1, S, S)
    lab, do, lo, hits = torch.zeros(1, 3, 4, dtype=torch.uint8), f32(1, S, S), torch.zeros(1, S, S, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def compose(B=1, Hs=3, Ws=4, S_=S, null=None, hits_=None):
        a = [ptr(fi), ptr(w), ptr(rd), ptr(lab), B, Hs, Ws, S_, ptr(do), ptr(lo), ptr(hits) if hits_ is None else hits_, None]
        if null is not None:
            a[null] = None
        return lib.sln_reproject_compose(*a)
    for kw in (dict(B=0), dict(B=65536), dict(Hs=1), dict(Ws=1), dict(Hs=4097, Ws=2050), dict(S_=0), dict(S_=4097), dict(hits_=C.c_void_p(hits.data_ptr() + 4)),
               dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=8), dict(null=9), dict(null=10)):
        assert compose(**kw) == -1, kw
    with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
        RP.compose(fi, w, rd, torch.zeros(1, 1, 4, dtype=torch.uint8), do, lo, hits)
    # the instance refuses sizes and devices itself
    for kw in (dict(Hs=1), dict(Ws=1), dict(S=0), dict(S=4097), dict(batch=0), dict(batch=65536), dict(Hs=4097, Ws=2050), dict(near=0.0), dict(gap=-1.0)):
        with pytest.raises(ValueError):
            RP.ObservedReprojector(**dict(dict(Hs=3, Ws=4, S=8, device="cpu"), **kw))
    with pytest.raises(L.SlnError, match="no CPU fallback"):
        RP.ObservedReprojector(3, 4, 8, device="cpu")
    with pytest.raises(ValueError):
        RP.reproject_torch(dep, lab.float(), k, P, K, 512.0, 8, None)
    with pytest.raises(ValueError):
        RP.faces_torch(dep, k, P, K, 0.0)


def test_abi_table_and_build_flags():
    L, B = pkg("_lib"), pkg("build")
    assert len(L.SIGNATURES["sln_reproject_faces"][1]) == 3 and len(L.SIGNATURES["sln_reproject_compose"][1]) == 12
    assert C.sizeof(L.SlnReproject) == 4 * 8 + 4 * 4 + 4 * 4
    assert "observed_reproject.hip" in B.sources() and "observed_reproject.hip" not in B.PER_FILE


# ------------------------------------------------------------------------------------------------------------------------------
# the measured figures (printed; the constants of test_observed_reproject_gpu.py are held to them)
# ------------------------------------------------------------------------------------------------------------------------------
def test_fp32_restatement_stays_inside_the_figure_the_kernel_is_allowed_four_times_of():
    import test_observed_reproject_gpu as G
    worst = 0.0
    for c in CASES:
        err, flips = OC.face_error(OC.torch_route(c, torch.float32)["faces_xyz"], OC.torch_route(c, torch.float64)["faces_xyz"])
        print("%s: fp32 torch against fp64, largest |d| / max(1, |want|) = %.3e" % (c["name"], err))
        assert flips == 0
        worst = max(worst, err)
    print("largest: %.3e (FP32_TORCH_ERR %.3e)" % (worst, G.FP32_TORCH_ERR))
    assert worst <= G.FP32_TORCH_ERR <= 2.0 * worst


def test_fp32_route_on_the_planes_stays_inside_its_figure():
    import test_observed_reproject_gpu as G
    worst = 0.0
    for c, b in _plane_frames():
        want, inside, _, _ = OC.closed_form(c, b)
        w = OC.torch_route(c, torch.float32)
        m = inside & (w["depth"][b] > 0)
        if bool(m.any()):
            err = float((w["depth"][b].double() - want)[m].abs().max())
            print("%s frame %d: float32 route against the closed form on %d pixels: %.3e" % (c["name"], b, int(m.sum()), err))
            worst = max(worst, err)
    print("largest: %.3e (PLANE_F32_ERR %.3e)" % (worst, G.PLANE_F32_ERR))
    assert worst <= G.PLANE_F32_ERR <= 2.0 * worst


def test_round_trip_of_the_recorded_render_under_the_float32_route():
    """tests/golden/observed_reproject_room.npz: the observation (observe() of a RefineScene render at S = 64) of the room the GPU test
    renders, recorded from the device.  Settled pixels - at least half the image - are all hit, carry the source's label, and the depth
    figure of the float32 route with the C rasterizer is what the device route is allowed four times of."""
    import test_observed_reproject_gpu as G
    from oracle import raster_ref
    RP = pkg("host.reproject")
    g = load_golden("observed_reproject_room")
    depth, labels = torch.from_numpy(g["depth"]), torch.from_numpy(g["labels"])
    S = OC.ROUND_TRIP_S
    assert depth.shape == (1, S, S)
    k_src, pose, K, orig = OC.round_trip_inputs(g["room"], S)
    ok = OC.settled(depth, labels)
    assert 2 * int(ok.sum()) >= S * S
    for dtype in (torch.float64, torch.float32):
        w = RP.reproject_torch(depth, labels, k_src, pose, K, orig, S, raster_ref.nmr_forward, dtype=dtype)
        hit = w["depth"] > 0
        assert not bool((ok & ~hit).any()) and torch.equal(w["labels"][ok], labels[ok])
        err = float((w["depth"] - depth)[ok].abs().max())
        print("%s route: %d settled pixels of %d, %d hits, largest depth error on the settled pixels %.3e" % (
            str(dtype).replace("torch.", ""), int(ok.sum()), S * S, int(w["hits"][0]), err))
    print("ROUND_TRIP_F32_ERR %.3e" % G.ROUND_TRIP_F32_ERR)
    assert err <= G.ROUND_TRIP_F32_ERR <= 2.0 * err
