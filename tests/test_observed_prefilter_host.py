"""Pre-filter of observed frames finer than the target, host side (host/reproject.py: prefilter_torch, prefilter_factor,
reproject_torch(prefilter=), the classes' checks; CPU-only): the torch definition against a plain per-block loop, planes against their
closed form at the coarse centres, the f = 1 identity over every float32 exponent, what the hand-made blocks are there for, the choice
of the factor, the whole float32 route on filtered frames, the refusals (which run before anything is launched, so they need no device)
and the measured figures the GPU test's allowance is a multiple of."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import observed_prefilter_cases as PC
import observed_reproject_cases as OC
from conftest import pkg

# Largest |depth / closed form - 1| of prefilter_torch over the plane frames of observed_prefilter_cases, the closed form being the
# plane's depth at the coarse pixel centres under k64 / f in float64: measured 6.861e-08 (the rounding of the float32 source depths; H2
# prints it per frame and holds this constant to at most twice the worst).
PLANE_CENTRE_REL_ERR = 7.0e-8


def _bits(a):
    return a.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# H1: the definition once more, block by block
# ------------------------------------------------------------------------------------------------------------------------------
def _loop_prefilter(depth, labels, k_src, f, gap):
    depth, labels = depth.numpy(), labels.numpy()
    B, Hs, Ws = depth.shape
    Hd, Wd, n = Hs // f, Ws // f, f * f
    gap = np.float32(gap)
    out_d, out_l = np.zeros((B, Hd, Wd), np.float32), np.zeros((B, Hd, Wd), np.uint8)
    counts = np.zeros((B, 3), np.int64)
    for b in range(B):
        for I in range(Hd):
            for J in range(Wd):
                px = [(depth[b, f * I + i, f * J + j], int(labels[b, f * I + i, f * J + j])) for i in range(f) for j in range(f)]
                readings = [d for d, _ in px if d > 0 and d <= np.float32(15.0)]
                r = len(readings)
                if 2 * r < n:
                    counts[b, 2] += 1
                    continue
                dref = sorted(readings)[(r - 1) // 2]
                total, m, votes = np.float64(0.0), 0, {}
                for d, l in px:
                    if not (d > 0 and d <= np.float32(15.0)):
                        continue
                    hi, lo = max(d, dref), min(d, dref)
                    if np.float32(hi - lo) > np.float32(gap * lo):
                        continue
                    total = total + np.float64(1.0) / np.float64(d)
                    m += 1
                    votes[l] = votes.get(l, 0) + 1
                out_d[b, I, J] = np.float32(np.float64(m) / total)
                out_l[b, I, J] = min(l for l in votes if votes[l] == max(votes.values()))
                counts[b, 0 if m == n else 1] += 1
    k_out = (k_src.numpy().astype(np.float32) / np.float32(f)).astype(np.float32)
    return out_d, out_l, k_out, counts


@pytest.mark.parametrize("name", PC.NAMES)
def test_prefilter_torch_against_a_plain_loop(name):
    """H1: depth bits, labels, k_out bits and counts"""
    c = PC.case(name)
    got = PC.filtered(c)
    with np.errstate(invalid="ignore"):
        want = _loop_prefilter(c["depth_src"], c["labels_src"], c["k_src"], c["f"], c["gap"])
    B, Hs, Ws = c["depth_src"].shape
    Hd, Wd = Hs // c["f"], Ws // c["f"]
    assert got[0].shape == (B, Hd, Wd) and got[0].dtype == torch.float32 and got[1].dtype == torch.uint8 and got[2].dtype == torch.float32
    assert got[3].dtype == torch.int64 and got[3].shape == (B, 3)
    assert torch.equal(_bits(got[0]), _bits(torch.from_numpy(want[0]))), "depth bits"
    assert torch.equal(got[1], torch.from_numpy(want[1])), "labels"
    assert torch.equal(_bits(got[2]), _bits(torch.from_numpy(want[2]))), "k_out bits"
    assert torch.equal(got[3], torch.from_numpy(want[3])), "counts"
    assert got[3].sum(1).tolist() == [Hd * Wd] * B, "counts sum to Hd * Wd"
    assert torch.equal((got[0] == 0), (got[0] <= 0)) and bool((got[1][got[0] == 0] == 0).all()), "no reading: 0.0 and label 0"


# ------------------------------------------------------------------------------------------------------------------------------
# H2: planes at the coarse centres
# ------------------------------------------------------------------------------------------------------------------------------
def test_planes_are_exact_at_the_coarse_centres():
    """H2: every block of a plane frame is full - a condition of the case - and the harmonic mean is the plane's depth at the centre"""
    worst, frames = 0.0, 0
    seen = set()
    for c, b in PC.plane_frames():
        depth, _, _, counts = PC.filtered(c)
        Hd, Wd = depth.shape[1:]
        if c["name"] == "poisoned_5x7_f2":
            assert (Hd, Wd) == (2, 3)
        assert counts[b].tolist() == [Hd * Wd, 0, 0], "%s frame %d: every block full" % (c["name"], b)
        n, cc = c["plane"][b]
        want = OC._plane_depth(Hd, Wd, c["k64"][b] / c["f"], n, cc)
        err = float(np.abs(depth[b].double().numpy() / want - 1.0).max())
        print("%s frame %d (f = %d): %d coarse pixels against the plane at their centres: %.3e relative" % (c["name"], b, c["f"], Hd * Wd, err))
        worst, frames = max(worst, err), frames + 1
        seen.add(c["f"])
        if c["plane"][b] is OC.FRONT:
            assert bool((depth[b] == 2.0).all()), "a fronto-parallel plane comes back exactly"
        if any(c["plane"][b] is p for p in (OC.SLANT, OC.MILD)):
            naive = c["depth_src"][b, :c["f"] * Hd, :c["f"] * Wd].double().reshape(Hd, c["f"], Wd, c["f"]).mean(dim=(1, 3)).numpy()
            assert float(np.abs(naive / want - 1.0).max()) > 4 * err, "the mean of z is biased on a slanted plane; the harmonic mean is not"
    print("largest: %.3e over %d frames (PLANE_CENTRE_REL_ERR %.3e)" % (worst, frames, PLANE_CENTRE_REL_ERR))
    assert seen >= {2, 3, 4, 8} and frames >= 6
    assert worst <= PLANE_CENTRE_REL_ERR <= 2.0 * worst


# ------------------------------------------------------------------------------------------------------------------------------
# H3: f = 1
# ------------------------------------------------------------------------------------------------------------------------------
def test_factor_one_keeps_the_bits_of_every_reading():
    """H3: (float)(1.0 / (1.0 / (double)d)) == d over all float32 exponents in (0, 15], denormals included; the rest becomes 0.0 / 0"""
    RP = pkg("host.reproject")
    rng = np.random.default_rng(5)
    mant = rng.integers(0, 1 << 23, (131, 64), dtype=np.int64)
    mant[:, 0] = 0; mant[:, 1] = (1 << 23) - 1
    bits = (np.arange(0, 131, dtype=np.int64)[:, None] << 23) | mant                   # exponent fields 0 .. 130: up to 2^3 * 1.m
    d = torch.from_numpy(bits.astype(np.int32)).view(torch.float32)
    nan = float("nan")
    extra = torch.tensor([[0.0, -0.0, nan, float("inf"), -float("inf"), -1.0, 15.0, 15.000001, 16.0, 1e30] + [1.0] * 54])
    d = torch.cat((d, extra), 0)[None]
    lab = torch.from_numpy(rng.integers(1, 256, tuple(d.shape)).astype(np.uint8))
    depth, labels, k_out, counts = RP.prefilter_torch(d, lab, torch.tensor([[500.0, 400.0, 320.3, 239.8]]), 1)
    reading = (d > 0) & (d <= 15.0)
    assert int(reading.sum()) > 130 * 64 and int((~reading).sum()) >= 8 and bool(reading[0, 0, 1:].all()), "denormals are readings"
    assert torch.equal(_bits(depth)[reading], _bits(d)[reading]) and torch.equal(labels[reading], lab[reading])
    assert bool((_bits(depth)[~reading] == 0).all()) and bool((labels[~reading] == 0).all())
    assert torch.equal(k_out, torch.tensor([[500.0, 400.0, 320.3, 239.8]]))
    assert counts.tolist() == [[int(reading.sum()), 0, int((~reading).sum())]]
    c = PC.case("identity_2x2_f1")
    depth, labels, _, counts = PC.filtered(c)
    assert depth.tolist() == [[[1.5, 0.0], [0.0, 15.0]]] and labels.tolist() == [[[7, 0], [0, 255]]] and counts.tolist() == [[2, 0, 2]]


# ------------------------------------------------------------------------------------------------------------------------------
# H4: what the hand-made blocks are there for, spelled out
# ------------------------------------------------------------------------------------------------------------------------------
def test_hand_made_blocks_say_what_the_definition_says():
    """H4"""
    RP = pkg("host.reproject")
    depth, labels, k_out, counts = PC.filtered(PC.case("blocks_4x4_f2"))
    assert depth[0].tolist() == [[2.0, 2.0], [2.0, 0.0]], "2 r == n is a reading, 2 r < n is none"
    assert labels[0].tolist() == [[5, 0], [5, 0]], "a tie goes to the smaller byte, 0 included"
    assert counts.tolist() == [[2, 1, 1]]
    # the remainder row and column are never read: the same as the frame without them
    c = PC.case("poisoned_5x7_f2")
    got = PC.filtered(c)
    crop = RP.prefilter_torch(c["depth_src"][:, :4, :6].contiguous(), c["labels_src"][:, :4, :6].contiguous(), c["k_src"], 2, c["gap"])
    assert bool(torch.isnan(c["depth_src"][0, 4]).all()) and bool((c["labels_src"][0, :, 6] == 255).all())
    assert all(torch.equal(a, b) for a, b in zip(got, crop)) and not bool(torch.isnan(got[0]).any()) and int(got[1].max()) <= 40
    # an odd factor: k_out is k_src / 3 in float32
    c = PC.case("plane_9x12_f3")
    assert torch.equal(PC.filtered(c)[2], c["k_src"] / torch.tensor(3.0))
    # blocks of 8 x 8
    c = PC.case("speckles_16x24_f8")
    depth, labels, _, counts = PC.filtered(c)
    src = c["depth_src"][0]
    assert labels[0].tolist() == [[6, 6, 6], [3, 11, 6]], "a speckle never names the block; the majority byte 9 belongs to non-members only"
    assert counts.tolist() == [[2, 4, 0]]
    for (I, J), lo, hi in (((0, 0), 1.5, 3.0), ((0, 1), 1.5, 3.0)):
        blk = src[8 * I:8 * I + 8, 8 * J:8 * J + 8]
        body = blk[(blk > lo) & (blk < hi)]
        assert body.numel() == 63 and float(body.min()) <= float(depth[0, I, J]) <= float(body.max()), "the speckle is no member"
    assert float(src[8:12, 0:8].min()) <= float(depth[0, 1, 0]) <= float(src[8:12, 0:8].max()) * 1.001
    assert float(src[8:12, 8:16].min()) <= float(depth[0, 1, 1]) <= float(src[8:12, 8:16].max()), "exactly half: the lower median is the nearer surface"
    # holes at random: every count of readings occurs, and so does every kind of block
    c = PC.case("holes_37x70_f2")
    d = c["depth_src"][0, :36, :70].reshape(18, 2, 35, 2)
    r = ((d > 0) & (d <= 15.0)).sum(dim=(1, 3))
    assert set(r.flatten().tolist()) == {0, 1, 2, 3, 4}
    depth, labels, _, counts = PC.filtered(c)
    assert torch.equal(depth[0] > 0, r >= 2) and all(int(x) > 20 for x in counts[0]) and float(depth.max()) == 15.0
    assert set(labels[0][depth[0] > 0].tolist()) == {0, 3, 41, 255}


def test_a_step_of_half_takes_the_nearer_surface_and_a_step_of_a_hundredth_is_one_surface():
    """H5: frames_48x64_f4.  Frame 1: every coarse depth is one of the two surfaces - never a value between -, the nearer one wherever it
    covers at least half the block.  Frame 2: a step of 1 % is inside the gap, every block is full."""
    c = PC.case("frames_48x64_f4")
    depth, labels, k_out, counts = PC.filtered(c)
    near = (c["depth_src"][1] == PC.NEAR_Z).reshape(12, 4, 16, 4).sum(dim=(1, 3))
    assert set(near[6:].flatten().tolist()) == set(range(17)) and near[:6, 7].tolist() == [8] * 6, "every share from none to all; exactly half"
    assert bool(((depth[1] == PC.NEAR_Z) | (depth[1] == PC.FAR_Z)).all())
    assert torch.equal(depth[1] == PC.NEAR_Z, near >= 8) and torch.equal(labels[1] == 21, near >= 8) and torch.equal(labels[1] == 22, near < 8)
    assert counts[1].tolist() == [int(((near == 0) | (near == 16)).sum()), int(((near > 0) & (near < 16)).sum()), 0]
    assert counts[2].tolist() == [12 * 16, 0, 0] and 2.0 < float(depth[2, 0, 8]) < 2.02
    assert labels[2, 1, 1] == 0 and labels[2, 2, 2] == 41 and labels[2, 3, 3] == 255 and labels[2, 4, 4] == 0, "bytes pass; 0 wins its tie with 7"
    assert len({tuple(k) for k in c["k_src"].tolist()}) == 3 and torch.equal(k_out, c["k_src"] / torch.tensor(4.0))


# ------------------------------------------------------------------------------------------------------------------------------
# H6: the choice of the factor
# ------------------------------------------------------------------------------------------------------------------------------
def test_prefilter_factor_on_hand_made_cameras():
    """H6"""
    RP = pkg("host.reproject")
    K = torch.tensor([[[300.0, 0.0, 256.0], [0.0, 280.0, 256.0], [0.0, 0.0, 1.0]]])
    k = lambda fx, fy: [fx, fy, 320.0, 240.0]
    # target pixels per unit of tangent: S * 300 / 512 = 150 at S = 256
    assert RP.prefilter_factor(torch.tensor([k(500.0, 500.0)]), K, 512.0, 256) == 3           # 500 / 150 = 3.33
    assert RP.prefilter_factor(torch.tensor([k(500.0, 449.0)]), K, 512.0, 256) == 2           # min(fx, fy)
    assert RP.prefilter_factor(torch.tensor([k(500.0, 450.0)]), K, 512.0, 256) == 3           # exactly 3.0
    assert RP.prefilter_factor(torch.tensor([k(500.0, 500.0), k(310.0, 900.0)]), K, 512.0, 256) == 2      # the coarsest frame decides
    assert RP.prefilter_factor(torch.tensor([[k(500.0, 500.0), k(0.0, 500.0)]]), K, 512.0, 256) == 3      # a padding frame is skipped
    assert RP.prefilter_factor(torch.tensor([k(0.0, 0.0)]), K, 512.0, 256) == 1
    assert RP.prefilter_factor(torch.tensor([k(100.0, 100.0)]), K, 512.0, 256) == 1           # a frame coarser than the target
    assert RP.prefilter_factor(torch.tensor([k(5000.0, 5000.0)]), K, 512.0, 256) == 8         # the clamp
    assert RP.prefilter_factor(torch.tensor([k(5000.0, 5000.0)]), K, 512.0, 256, fmax=4) == 4
    assert RP.prefilter_factor(torch.tensor([k(500.0, 500.0)]), K, 512.0, 64) == 8            # 500 / 37.5
    K2 = torch.cat((K, K * torch.tensor([2.0, 2.0, 1.0])[:, None]), 0)
    assert RP.prefilter_factor(torch.tensor([k(1250.0, 1250.0)]), K, 512.0, 256) == 8 and \
        RP.prefilter_factor(torch.tensor([k(1250.0, 1250.0)]), K2, 512.0, 256) == 4             # the finest target decides: 1250 / 300 = 4.17
    for bad in (dict(orig_size=0.0), dict(S=0), dict(fmax=0), dict(fmax=9)):
        with pytest.raises(ValueError):
            RP.prefilter_factor(torch.tensor([k(500.0, 500.0)]), K, **dict(dict(orig_size=512.0, S=256), **bad))
    # the cases' own factors keep a coarse pixel at least as fine as the target on the axis
    for name in PC.ROUTE_NAMES:
        c = PC.case(name)
        assert RP.prefilter_factor(c["k_src"], c["K_tgt"], c["orig_size"], c["S"]) >= 1


# ------------------------------------------------------------------------------------------------------------------------------
# H7, H8: the whole float32 route on filtered frames
# ------------------------------------------------------------------------------------------------------------------------------
def test_fp32_route_on_filtered_planes_stays_inside_its_figure():
    """H7: the figure the device route is allowed four times of (PREFILTER_PLANE_F32_ERR of test_observed_prefilter_gpu.py)"""
    import test_observed_prefilter_gpu as G
    worst, checked = 0.0, 0
    for name in PC.ROUTE_NAMES:
        c = PC.case(name)
        t = PC.torch_route(c, torch.float32)
        Hd, Wd = PC.filtered(c)[0].shape[1:]
        assert t["faces_xyz"].shape[1] == 2 * (Hd - 1) * (Wd - 1), "the route runs on the coarse frame"
        for b, plane in enumerate(c["plane"]):
            if plane is None:
                continue
            want, inside, _, _ = OC.closed_form(PC.coarse(c), b)
            hit = t["depth"][b] > 0
            assert not bool((inside & ~hit).any()), "a plane is hit on every inside pixel"
            err = float((t["depth"][b].double() - want)[inside].abs().max())
            print("%s frame %d (f = %d): float32 route on the filtered frame against the closed form on %d pixels: %.3e" % (name, b, c["f"], int(inside.sum()), err))
            worst, checked = max(worst, err), checked + int(inside.sum())
    print("largest: %.3e on %d pixels (PREFILTER_PLANE_F32_ERR %.3e)" % (worst, checked, G.PREFILTER_PLANE_F32_ERR))
    assert checked >= 300
    assert worst <= G.PREFILTER_PLANE_F32_ERR <= 2.0 * worst


def test_two_surfaces_are_never_blended_on_the_way_to_the_target():
    """H8: frame 1 of frames_48x64_f4 through the float32 route: its pose moves along z only, so the target sees the surfaces at
    2 + tz and 3 + tz; no target pixel lies strictly between them by more than the route's figure"""
    import test_observed_prefilter_gpu as G
    c = PC.case("frames_48x64_f4")
    d = PC.torch_route(c, torch.float32)["depth"][1].double()
    lo, hi = PC.NEAR_Z + PC.STEP_POSE_TZ, PC.FAR_Z + PC.STEP_POSE_TZ
    fig = G.PREFILTER_PLANE_F32_ERR
    between = (d > lo + fig) & (d < hi - fig)
    assert int((d > 0).sum()) * 4 >= c["S"] ** 2 and int(((d - lo).abs() <= fig).sum()) > 20 and int(((d - hi).abs() <= fig).sum()) > 20
    assert not bool(between.any()), d[between]


def test_reproject_views_torch_takes_the_keyword():
    """H9: V frames per room through the filtered route equal the route on prefilter_torch's outputs"""
    from oracle import raster_ref
    RP = pkg("host.reproject")
    c = PC.case("frames_48x64_f4")
    args = (c["pose"][None], c["K_tgt"][:1], c["orig_size"], c["S"], raster_ref.nmr_forward)
    got = RP.reproject_views_torch(c["depth_src"][None], c["labels_src"][None], c["k_src"][None], *args, dtype=torch.float32, prefilter=4)
    d, l, k, _ = PC.filtered(c)
    want = RP.reproject_views_torch(d[None], l[None], k[None], *args, dtype=torch.float32)
    for key in ("depth", "labels", "source", "count", "agree", "hits", "wins"):
        assert torch.equal(got[key], want[key]), key
    assert int(got["hits"][0]) > 0
    one = RP.reproject_views_torch(c["depth_src"][None], c["labels_src"][None], c["k_src"][None], *args, dtype=torch.float32, prefilter=1)
    base = RP.reproject_views_torch(c["depth_src"][None], c["labels_src"][None], c["k_src"][None], *args, dtype=torch.float32)
    assert torch.equal(one["depth"], base["depth"]) and one["faces_xyz"].shape[1] == 2 * 47 * 63


# ------------------------------------------------------------------------------------------------------------------------------
# H10: refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_before_any_launch():
    """H10: host tensors stand in for the device buffers; every call below returns before a launch and none of the buffers is read"""
    RP, L = pkg("host.reproject"), pkg("_lib")
    B, Hs, Ws, f = 2, 6, 8, 2
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    d, l, k = f32(B, Hs, Ws), torch.zeros(B, Hs, Ws, dtype=torch.uint8), f32(B, 4)
    me = types.SimpleNamespace(batch=B, Hs=Hs, Ws=Ws, device=torch.device("cpu"))
    check = lambda *a: RP.ObservedPrefilter.check(me, *a)
    check(d, l, k)                                                   # sound arguments pass
    for args in ((d.double(), l, k), (d, l.to(torch.int32), k), (d.numpy(), l, k), (d[:1].contiguous(), l, k), (d, l[:, :2].contiguous(), k),
                 (d, l, k[:, :3].contiguous()), (d.transpose(1, 2).contiguous().transpose(1, 2), l, k), (d, l, k.to("meta"))):
        with pytest.raises(ValueError):
            check(*args)
    for kw in (dict(f=0), dict(f=9), dict(f=2.5), dict(Hs=1), dict(Ws=1), dict(batch=0), dict(batch=65536), dict(gap=-1.0), dict(gap=float("nan"))):
        with pytest.raises(ValueError):
            RP.ObservedPrefilter(**dict(dict(Hs=6, Ws=8, f=2, batch=1, device="cpu"), **kw))
    with pytest.raises(L.SlnError, match="no CPU fallback"):
        RP.ObservedPrefilter(6, 8, 2, device="cpu")
    # the routes' keyword: the coarse frame must be at least 2 x 2
    for kw in (dict(prefilter=0), dict(prefilter=9), dict(prefilter=4), dict(prefilter=1.5)):
        with pytest.raises(ValueError):
            RP.ObservedReprojector(**dict(dict(Hs=6, Ws=8, S=8, batch=1, device="cpu"), **kw))
        with pytest.raises(ValueError):
            RP.ObservedFuser(**dict(dict(Hs=6, Ws=8, S=8, rooms=1, views=2, device="cpu"), **kw))
    with pytest.raises(L.SlnError, match="no CPU fallback"):
        RP.ObservedReprojector(6, 8, 8, device="cpu", prefilter=3)
    # the torch definition
    for kw in (dict(f=0), dict(f=9), dict(f=7), dict(f=2, gap=-0.1), dict(f=2, gap=float("nan"))):
        with pytest.raises(ValueError):
            RP.prefilter_torch(d, l, k, **kw)
    with pytest.raises(ValueError):
        RP.prefilter_torch(d, l.float(), k, 2)
    with pytest.raises(ValueError):
        RP.prefilter_torch(d, l, f32(B + 1, 4), 2)
    with pytest.raises(ValueError):
        RP.reproject_torch(d, l, k, f32(B, 3, 4), f32(B, 3, 3), 512.0, 8, None, prefilter=4)
    # the entry point
    lib = L.lib()
    Hd, Wd = Hs // f, Ws // f
    out = PC.junk(B, Hd, Wd)
    counts = torch.full((3 * B + 1,), -3, dtype=torch.int64)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(B_=B, Hs_=Hs, Ws_=Ws, f_=f, gap=0.05, null=None, **at):
        a = [ptr(d), ptr(l), ptr(k), B_, Hs_, Ws_, f_, gap, ptr(out["depth"]), ptr(out["labels"]), ptr(out["k_out"]), ptr(counts), None]
        if null is not None:
            a[null] = None
        for i, v in at.items():
            a[int(i[1:])] = v
        return lib.sln_observed_prefilter(*a)
    for kw in (dict(null=0), dict(null=1), dict(null=2), dict(null=8), dict(null=9), dict(null=10), dict(B_=0), dict(B_=65536), dict(f_=0), dict(f_=9),
               dict(f_=-2), dict(Hs_=1), dict(Ws_=1), dict(f_=8), dict(gap=-0.01), dict(gap=float("nan")), dict(a11=C.c_void_p(counts.data_ptr() + 4)),
               dict(a8=C.c_void_p(out["depth"].data_ptr() + 2))):
        assert call(**kw) == -1, kw
    fresh = PC.junk(B, Hd, Wd)
    assert all(torch.equal(out[key], fresh[key]) for key in out) and bool((counts == -3).all()), "nothing written"
    with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
        RP.prefilter(d, l, k, 9, 0.05, out["depth"], out["labels"], out["k_out"])
    assert len(L.SIGNATURES["sln_observed_prefilter"][1]) == 13
    build = pkg("build")
    assert "observed_prefilter.hip" in build.PER_FILE and "observed_prefilter.hip" in build.sources()
    assert "-ffp-contract=off" in build.PER_FILE["observed_prefilter.hip"]
