"""Fusion of several observed frames per room, host side (host/reproject.py: fuse_torch, reproject_views_torch, ObservedFuser.check;
CPU-only): the torch definition against a plain loop on hand-made maps, against compose_torch at V = 1, under a permutation of the
frames, on a nearer surface in front of a farther one, on a plane cut in two against the uncut plane, the argument checks (which run
before anything is launched, so they need no device) and the measured figure the GPU test's allowance is a multiple of."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import observed_fuse_cases as FC
from conftest import pkg


def _bits(a):
    return a.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# H1: the definition once more, pixel by pixel and frame by frame
# ------------------------------------------------------------------------------------------------------------------------------
def _loop_fuse(m):
    R, V, Hs, Ws, S, F = (m[k] for k in ("R", "V", "Hs", "Ws", "S", "F"))
    fi, w, dep, lab = m["face_index"].numpy(), m["weight"].numpy(), m["raster_depth"].numpy(), m["labels_src"].numpy()
    gap = np.float32(m["gap"])
    px = {(0, 0): (0, 0), (0, 1): (1, 0), (0, 2): (0, 1), (1, 0): (1, 1), (1, 1): (0, 1), (1, 2): (1, 0)}       # (slot, corner) -> pixel of the cell
    out = dict(depth=np.full((R, S, S), -1.0, np.float32), labels=np.zeros((R, S, S), np.uint8), source=np.zeros((R, S, S), np.uint8),
               count=np.zeros((R, S, S), np.uint8), agree=np.zeros((R, S, S), np.uint8), hits=np.zeros(R, np.int64), wins=np.zeros((R, V), np.int64))
    for r in range(R):
        for y in range(S):
            for x in range(S):
                seen = []
                for v in range(V):
                    b = r * V + v
                    k, d = int(fi[b, y, x]), dep[b, y, x]
                    if 0 <= k < F and not np.isnan(w[b, y, x]).any() and not np.isnan(d):
                        seen.append((v, k, d))
                if not seen:
                    continue
                win = seen[0]
                for s in seen[1:]:
                    if s[2] < win[2]:
                        win = s
                v, k, dmin = win
                ws = w[r * V + v, y, x]
                corner = 1 if ws[1] > ws[0] else 0
                if ws[2] > ws[corner]:
                    corner = 2
                ci, cj = (k // 2) // (Ws - 1), (k // 2) % (Ws - 1)
                di, dj = px[(k % 2, corner)]
                row = S - 1 - y
                out["depth"][r, row, x] = dmin
                out["labels"][r, row, x] = lab[r * V + v, ci + di, cj + dj]
                out["source"][r, row, x] = v + 1
                out["count"][r, row, x] = len(seen)
                with np.errstate(invalid="ignore"):
                    out["agree"][r, row, x] = sum(1 for s in seen if not (np.float32(s[2] - dmin) > np.float32(gap * dmin)))
                out["hits"][r] += 1
                out["wins"][r, v] += 1
    return out


def test_fuse_torch_against_a_plain_loop_on_hand_made_maps():
    """H1"""
    RP = pkg("host.reproject")
    m = FC.maps()
    got = RP.fuse_torch(m["face_index"], m["weight"], m["raster_depth"], m["labels_src"], m["V"], m["gap"])
    want = _loop_fuse(m)
    R, V, S, F = m["R"], m["V"], m["S"], m["F"]
    for k, dt in (("depth", torch.float32), ("labels", torch.uint8), ("source", torch.uint8), ("count", torch.uint8), ("agree", torch.uint8),
                  ("hits", torch.int64), ("wins", torch.int64)):
        assert got[k].dtype == dt and got[k].shape == want[k].shape, k
        if k == "depth":
            assert torch.equal(_bits(got[k]), _bits(torch.from_numpy(want[k]))), k
        else:
            assert torch.equal(got[k], torch.from_numpy(want[k])), k
    assert torch.equal(got["wins"].sum(1), got["hits"]) and torch.equal(got["hits"], (got["source"] > 0).sum(dim=(1, 2)))
    # what the definition says about raster row 0 of room 0 (the planes' row S - 1), spelled out: (depth, source, count, agree) per pixel
    dmin, d_at, d_above = m["edge"]
    assert np.float32(d_at) - np.float32(dmin) == np.float32(m["gap"]) * np.float32(dmin) and d_above > d_at
    row = lambda k: got[k][0, S - 1, :8].tolist()
    assert row("depth") == [-1.0, 2.0, 5.0, 2.5, 1.5, dmin, 1.0, 1.0]
    assert row("source") == [0, 3, 2, 2, 1, 1, 4, 3], "NaN weights on the nearest: the next one wins; equal depths go to the lowest v"
    assert row("count") == [0, 3, 3, 4, 4, 4, 4, 3], "a NaN depth and NaN weights do not contribute"
    assert row("agree") == [0, 1, 1, 2, 3, 2, 1, 2], "exactly at dmin + gap * dmin agrees, one ulp above does not"
    lab = m["labels_src"]
    # frame v's face on this row is (3, 10, 21, F - 1)[v], weights (0.2, 0.3, 0.5): corner 2 - c of slot (a, b, c), b of slot (d, c, b)
    cell = lambda k: ((k // 2) // (m["Ws"] - 1), (k // 2) % (m["Ws"] - 1))
    for x, v in ((1, 2), (2, 1), (3, 1), (4, 0), (5, 0), (6, 3), (7, 2)):
        k = (3, 10, 21, F - 1)[v]
        ci, cj = cell(k)
        di, dj = (1, 0) if k % 2 else (0, 1)
        assert int(got["labels"][0, S - 1, x]) == int(lab[v, ci + di, cj + dj]), (x, v)
    assert int(got["labels"][0, S - 1, 0]) == 0
    # room 1: every frame misses
    assert int(got["hits"][1]) == 0 and got["wins"][1].tolist() == [0] * V and bool((got["depth"][1] == -1).all())
    assert all(int(got[k][1].max()) == 0 for k in ("labels", "source", "count", "agree"))
    # the sprinkled rows hold what they are there for: ties of two and more, frames lost to each rule, every frame a winner somewhere
    assert set(got["source"][0].flatten().tolist()) == {0, 1, 2, 3, 4} and int((got["agree"][0] >= 2).sum()) > 20
    assert int((got["count"][0, S - 20:S - 8] < V).sum()) > 100


# ------------------------------------------------------------------------------------------------------------------------------
# H2 - H5: properties on the rasterized cases
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["maps", "one_view_48x64_s64"])
def test_one_view_is_compose(where):
    """H2"""
    RP = pkg("host.reproject")
    if where == "maps":
        m = FC.maps()
        fi, w, dep, lab = m["face_index"], m["weight"], m["raster_depth"], m["labels_src"]
    else:
        c = FC.case(where)
        t = FC.torch_route(c, torch.float32)
        fi, w, dep, lab = t["face_index"], t["weight"], t["raster_depth"], c["labels_src"].reshape(-1, *c["labels_src"].shape[2:])
    got = RP.fuse_torch(fi, w, dep, lab, 1, 0.05)
    d, l, hits = RP.compose_torch(fi, w, torch.where(torch.isnan(dep), torch.zeros_like(dep), dep) if where == "maps" else dep, lab)
    if where == "maps":
        # (compose has no rule for a NaN depth on a hit: the hand-made maps hold some, and fusion drops them - compare where there is none)
        nan_hit = torch.flip(torch.isnan(dep), [1]) & (d != -1)
        assert int(nan_hit.sum()) > 0 and bool((got["source"][nan_hit] == 0).all())
        keep = ~nan_hit
        assert torch.equal(_bits(got["depth"])[keep], _bits(d)[keep]) and torch.equal(got["labels"][keep], l[keep])
        assert torch.equal(got["hits"], hits - nan_hit.sum(dim=(1, 2)))
    else:
        assert not bool(torch.isnan(dep).any())
        assert torch.equal(_bits(got["depth"]), _bits(d)) and torch.equal(got["labels"], l) and torch.equal(got["hits"], hits)
        assert int(hits[0]) > 0 and int(hits[2]) > 0
    hit = (got["depth"] != -1).to(torch.uint8)
    assert torch.equal(got["source"], hit) and torch.equal(got["count"], hit) and torch.equal(got["agree"], hit)
    assert torch.equal(got["wins"][:, 0], got["hits"])


def test_permuting_the_frames_permutes_source_and_wins_only():
    """H3"""
    RP = pkg("host.reproject")
    c = FC.case("two_rooms_18x34_s32")
    t = FC.torch_route(c, torch.float32)
    R, V, S = c["R"], c["V"], c["S"]
    perm = [2, 0, 1]
    idx = torch.tensor([r * V + v for r in range(R) for v in perm])
    lab = c["labels_src"].reshape(R * V, *c["labels_src"].shape[2:])
    got = RP.fuse_torch(t["face_index"][idx], t["weight"][idx], t["raster_depth"][idx], lab[idx], V, c["gap"])
    assert torch.equal(_bits(got["depth"]), _bits(t["depth"])) and torch.equal(got["count"], t["count"]) and torch.equal(got["agree"], t["agree"])
    assert torch.equal(got["hits"], t["hits"])
    # new frame v is old frame perm[v]: a pixel old frame perm[v] won is won by v now - wherever no two contributing depths are equal
    d = torch.flip(t["raster_depth"].reshape(R, V, S, S), [2])
    tied = (((d == t["depth"][:, None]) & (t["depth"][:, None] != -1)).sum(1) > 1)
    old_of_new = torch.tensor([0] + [p + 1 for p in perm])
    assert torch.equal(old_of_new[got["source"].long()][~tied], t["source"].long()[~tied])
    if not bool(tied.any()):
        assert torch.equal(got["wins"], t["wins"][:, perm])
    assert int(t["hits"][0]) > 0 and int(t["hits"][1]) > 0 and int((t["count"] >= 2).sum()) > 50, "the case fuses something"
    assert t["wins"][1, :2].tolist() == [0, 0], "a frame seen from behind and a frame with fx = 0 win nothing"
    assert all(int(x) > 0 for x in t["wins"][0]), "every frame of room 0 wins somewhere"


def test_the_nearer_surface_wins():
    """H4"""
    c = FC.case("near_wins_18x34_s32")
    t = FC.torch_route(c, torch.float32)
    S = c["S"]
    F = 2 * 17 * 33
    fi1 = t["face_index"][1]
    contributes = torch.flip((fi1 >= 0) & (fi1 < F), [0])
    src, count, agree = t["source"][0], t["count"][0], t["agree"][0]
    assert int(contributes.sum()) > S * S // 8 and int((~contributes).sum()) > S * S // 8
    assert not bool((src == 3).any()), "a copy of frame 0 never wins against frame 0"
    assert torch.equal(src == 2, contributes)
    assert bool((count[contributes] == 3).all()) and bool((agree[contributes] == 1).all())
    assert torch.equal(agree[~contributes], count[~contributes]) and bool((count[~contributes & (src > 0)] == 2).all())
    assert t["wins"][0].tolist() == [int((src == 1).sum()), int((src == 2).sum()), 0]


def test_a_plane_cut_in_two_is_the_whole_plane():
    """H5"""
    c = FC.case("split_plane_18x34_s32")
    Hs, Ws = c["depth_src"].shape[2:]
    for dtype in (torch.float32, torch.float64):
        t, w = FC.torch_route(c, dtype), FC.whole_route(c, dtype)
        hit = w["depth"][0] != -1
        seam = FC.seam(w["face_index"], Hs, Ws, c["cut"])[0]
        assert int(hit.sum()) * 4 >= c["S"] ** 2 and bool((seam & ~hit).sum() == 0)
        assert 0 < int(seam.sum()) <= 0.15 * int(hit.sum()), "the excluded set, on the whole-frame route alone"
        assert torch.equal(_bits(t["depth"][0]), _bits(w["depth"][0])), "depth: every pixel"
        assert torch.equal(t["labels"][0][~seam], w["labels"][0][~seam])
        assert int(t["count"].max()) <= 2 and not bool(((t["count"][0] == 2) & ~seam).any())
        assert torch.equal(t["hits"], w["hits"]) and int(t["wins"][0, 0]) > 0 and int(t["wins"][0, 1]) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# H6: the measured figure (printed; FUSE_PLANE_F32_ERR of test_observed_fuse_gpu.py is held to it)
# ------------------------------------------------------------------------------------------------------------------------------
def test_fp32_route_on_the_fused_planes_stays_inside_its_figure():
    """H6"""
    import test_observed_fuse_gpu as G
    worst, checked = 0.0, 0
    for c in FC.cases():
        t = FC.torch_route(c, torch.float32)
        for b, want, m in FC.plane_pixels(c, t):
            if bool(m.any()):
                r = b // c["V"]
                err = float((t["depth"][r].double() - want)[m].abs().max())
                print("%s frame %d: float32 route against the closed form of the winner's plane on %d pixels: %.3e" % (c["name"], b, int(m.sum()), err))
                worst, checked = max(worst, err), checked + int(m.sum())
    print("largest: %.3e on %d pixels (FUSE_PLANE_F32_ERR %.3e)" % (worst, checked, G.FUSE_PLANE_F32_ERR))
    assert checked >= 1000
    assert worst <= G.FUSE_PLANE_F32_ERR <= 1.1 * worst


# ------------------------------------------------------------------------------------------------------------------------------
# H7: refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_refuse_before_any_launch():
    """H7: host tensors stand in for the device buffers; ``check`` reads the instance's sizes, scalars and device only, so a stand-in
    for the instance carries them here.  Every call below returns before a launch; none of the buffers is read."""
    RP, L = pkg("host.reproject"), pkg("_lib")
    R, V, Hs, Ws = 2, 3, 4, 5
    me = types.SimpleNamespace(rooms=R, views=V, Hs=Hs, Ws=Ws, near=0.1, gap=0.05, device=torch.device("cpu"))
    check = lambda *a: RP.ObservedFuser.check(me, *a)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    d, l, k, P, K = f32(R, V, Hs, Ws), torch.zeros(R, V, Hs, Ws, dtype=torch.uint8), f32(R, V, 4), f32(R, V, 3, 4), f32(R, 3, 3)
    check(d, l, k, P, K, 512.0)                                      # sound arguments pass
    bad = [(d.double(), l, k, P, K, 512.0), (d, l.to(torch.int32), k, P, K, 512.0), (d.numpy(), l, k, P, K, 512.0), (d.reshape(R * V, Hs, Ws), l, k, P, K, 512.0),
           (d, l[:, :2].contiguous(), k, P, K, 512.0), (d, l, k.reshape(R * V, 4), P, K, 512.0), (d, l, k, P[..., :3].contiguous(), K, 512.0),
           (d, l, k, P, f32(R * V, 3, 3), 512.0), (d, l, k, P, f32(R, V, 3, 3), 512.0), (d, l, k, P.transpose(2, 3).contiguous().transpose(2, 3), K, 512.0),
           (d.transpose(2, 3).contiguous().transpose(2, 3), l, k, P, K, 512.0), (d, l, k, P, K, 0.0), (d, l, k, P, K, -512.0), (d, l, k, P, K, float("nan")),
           (d, l, k, P, K.to("meta"), 512.0)]
    for args in bad:
        with pytest.raises(ValueError):
            check(*args)
    # the instance refuses sizes and scalars itself, then anything that is not the device
    for kw in (dict(Hs=1), dict(Ws=1), dict(S=0), dict(S=4097), dict(rooms=0), dict(views=0), dict(views=256), dict(rooms=258, views=255), dict(Hs=4097, Ws=2050),
               dict(near=0.0), dict(gap=-1.0), dict(gap=float("nan"))):
        with pytest.raises(ValueError):
            RP.ObservedFuser(**dict(dict(Hs=3, Ws=4, S=8, rooms=1, views=2, device="cpu"), **kw))
    with pytest.raises(L.SlnError, match="no CPU fallback"):
        RP.ObservedFuser(3, 4, 8, rooms=1, views=2, device="cpu")
    # the torch routes
    S = 8
    fi, w, rd = torch.zeros(R * V, S, S, dtype=torch.int32), f32(R * V, S, S, 3), f32(R * V, S, S)
    lab = l.reshape(R * V, Hs, Ws)
    for kw in (dict(V=0), dict(V=4), dict(V=256), dict(V=3, gap=-0.1), dict(V=3, gap=float("nan"))):
        with pytest.raises(ValueError):
            RP.fuse_torch(fi, w, rd, lab, **kw)
    with pytest.raises(ValueError):
        RP.reproject_views_torch(d, l.float(), k, P, K, 512.0, S, None)
    with pytest.raises(ValueError):
        RP.reproject_views_torch(d, l, k, P, f32(R * V, 3, 3), 512.0, S, None)
    # the entry point
    lib = L.lib()
    do, hits, wins = f32(R, S, S), torch.zeros(R + 1, dtype=torch.int64), torch.zeros(R * V + 1, dtype=torch.int64)
    u8 = [torch.zeros(R, S, S, dtype=torch.uint8) for _ in range(4)]
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def fuse(R_=R, V_=V, Hs_=Hs, Ws_=Ws, S_=S, gap=0.05, null=None, **at):
        a = [ptr(fi), ptr(w), ptr(rd), ptr(lab), R_, V_, Hs_, Ws_, S_, gap, ptr(do), ptr(u8[0]), ptr(u8[1]), ptr(u8[2]), ptr(u8[3]), ptr(hits), ptr(wins), None]
        if null is not None:
            a[null] = None
        for i, v in at.items():
            a[int(i[1:])] = v
        return lib.sln_reproject_fuse(*a)
    for kw in (dict(R_=0), dict(V_=0), dict(V_=256), dict(R_=258, V_=255), dict(R_=65536, V_=1), dict(Hs_=1), dict(Ws_=1), dict(S_=0), dict(S_=4097),
               dict(Hs_=4097, Ws_=2050), dict(gap=-0.01), dict(gap=float("nan")), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=10),
               dict(null=11), dict(null=15), dict(a15=C.c_void_p(hits.data_ptr() + 4)), dict(a16=C.c_void_p(wins.data_ptr() + 4)),
               dict(a10=C.c_void_p(do.data_ptr() + 2))):
        assert fuse(**kw) == -1, kw
    assert 257 * 255 == 65535 < 258 * 255
    with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
        RP.fuse(fi, w, rd, lab, V, -1.0, do, u8[0], hits)
    with pytest.raises(ValueError):
        RP.fuse(fi, w, rd, lab, 4, 0.05, do, u8[0], hits)
    assert len(L.SIGNATURES["sln_reproject_fuse"][1]) == 18
    assert "observed_fuse.hip" in pkg("build").sources()
