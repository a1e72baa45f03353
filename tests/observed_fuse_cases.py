"""Hand-made cases for the fusion of several observed frames per room (host/reproject.py: fuse_torch, ObservedFuser;
csrc/observed_fuse.hip): CPU tensors only, built with the helpers and planes of observed_reproject_cases and shared by
test_observed_fuse_host.py (the torch definition against a plain loop and against properties) and test_observed_fuse_gpu.py (the kernel
against the torch definition).

A rasterized case is a dict: ``name``, ``R``, ``V``, ``depth_src`` [R, V, Hs, Ws] float32, ``labels_src`` [R, V, Hs, Ws] uint8, ``k_src``
[R, V, 4], ``pose`` [R, V, 3, 4], ``K_tgt`` [R, 3, 3] (the room's), ``orig_size``, ``S``, ``near``, ``far``, ``gap`` and ``plane`` (a list of
R * V entries, frame r * V + v: (n, c) of the surface n . p = c in source camera coordinates, or None).  ``frames(c)`` is the same case
as R * V single frames in the layout observed_reproject_cases.closed_form reads.  ``split_plane_18x34_s32`` carries ``whole``: the uncut
frame as a one-frame case of observed_reproject_cases' layout, and ``cut``: the column it was cut at.

``maps()`` is a set of rasterizer maps made by hand, without a rasterizer: R 2, V 4, frames of 5 x 7, S = 33.
"""
import numpy as np
import torch

import observed_reproject_cases as OC

_CACHE = {}
NAMES = ["split_plane_18x34_s32", "near_wins_18x34_s32", "two_rooms_18x34_s32", "nothing_3x5_s16", "one_view_48x64_s64"]
CUT = 16                                                             # the face kernel's tile edge


def _fuse_case(name, S, rooms, K_of=0):
    """rooms: a list of R lists of V frames (observed_reproject_cases._frame dicts); the room's K_tgt is that of its frame ``K_of``"""
    R, V = len(rooms), len(rooms[0])
    assert all(len(r) == V for r in rooms)
    flat = OC._case(name, S, [f for r in rooms for f in r])
    Hs, Ws = flat["depth_src"].shape[1:]
    c = dict(flat, R=R, V=V, depth_src=flat["depth_src"].reshape(R, V, Hs, Ws).contiguous(), labels_src=flat["labels_src"].reshape(R, V, Hs, Ws).contiguous(),
             k_src=flat["k_src"].reshape(R, V, 4).contiguous(), pose=flat["pose"].reshape(R, V, 3, 4).contiguous(),
             K_tgt=flat["K_tgt"].reshape(R, V, 3, 3)[:, K_of].contiguous())
    del c["shows"]
    return c


def _from(case, b):
    """frame b of a case of observed_reproject_cases, as a frame dict"""
    return dict(depth=case["depth_src"][b].numpy().copy(), labels=case["labels_src"][b].numpy().copy(), k=case["k_src"][b].double().numpy(),
                pose=case["pose"][b].double().numpy(), K=case["K_tgt"][b].double().numpy(), plane=case["plane"][b], shows=case["shows"][b])


def _build():
    rng = np.random.default_rng(77)
    out = []
    Hs, Ws = 18, 34
    moved = OC._pose(-0.05, 0.1, (0.2, -0.1, 0.3))
    # one plane, cut in two at the tile edge: frame 0 keeps the readings of the columns <= CUT, frame 1 those of the columns >= CUT
    whole = OC._frame(rng, Hs, Ws, OC.MILD, moved, fl=320.0)
    left, right = dict(whole, depth=whole["depth"].copy(), labels=whole["labels"].copy()), dict(whole, depth=whole["depth"].copy(), labels=whole["labels"].copy())
    left["depth"][:, CUT + 1:] = 0.0; left["labels"][:, CUT + 1:] = 0
    right["depth"][:, :CUT] = 0.0; right["labels"][:, :CUT] = 0
    c = _fuse_case("split_plane_18x34_s32", 32, [[left, right]])
    c["whole"], c["cut"] = OC._case("split_plane_whole_18x34_s32", 32, [whole]), CUT
    out.append(c)
    # one camera and pose: a front plane at 2.5, a front plane at 2.0 with readings in the columns < 20 only, the first frame again
    pose = OC._pose(0.04, -0.08, (-0.15, 0.1, 0.25))
    far_plane, near_plane = (np.array([0.0, 0.0, 1.0]), 2.5), (np.array([0.0, 0.0, 1.0]), 2.0)
    n0 = OC._frame(rng, Hs, Ws, far_plane, pose)
    n1 = dict(OC._frame(rng, Hs, Ws, near_plane, pose), K=n0["K"])
    n1["depth"][:, 20:] = 0.0
    n2 = dict(n0, depth=n0["depth"].copy(), labels=n0["labels"].copy())
    out.append(_fuse_case("near_wins_18x34_s32", 32, [[n0, n1, n2]]))
    # two rooms.  Room 0: the three frames of tile_edge_18x34_s32 with their own cameras and poses (NaN, inf, 0, negative and 15.5 depths,
    # the bytes 0 / 41 / 255).  Room 1: a frame seen from behind, a frame with fx = 0, a sound frame
    t = OC.case("tile_edge_18x34_s32")
    behind = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.array([[0.0], [0.0], [6.0]])], 1)
    bad = OC._k_src(Hs, Ws); bad[0] = 0.0
    r1 = [OC._frame(rng, Hs, Ws, OC.SLANT, behind, shows=False), OC._frame(rng, Hs, Ws, OC.FRONT, shows=False, k_given=bad, keep_plane=False),
          OC._frame(rng, Hs, Ws, OC.GENTLE, OC._pose(0.02, 0.05, (0.1, 0.05, 0.15)), fl=310.0)]
    out.append(_fuse_case("two_rooms_18x34_s32", 32, [[_from(t, 0), _from(t, 1), _from(t, 2)], r1], K_of=2))
    out[-1]["K_tgt"][0] = t["K_tgt"][0]
    # no frame shows anything: no reading anywhere, and fx = 0
    n = OC.case("nothing_to_show_3x5_s16")
    out.append(_fuse_case("nothing_3x5_s16", 16, [[_from(n, 0), _from(n, 1)]]))
    # V = 1: the frames of frames_48x64_s64, a room each
    f = OC.case("frames_48x64_s64")
    out.append(_fuse_case("one_view_48x64_s64", 64, [[_from(f, 0)], [_from(f, 1)], [_from(f, 2)]]))
    return out


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = _build()
    return _CACHE["cases"]


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def frames(c):
    """the case as R * V single frames, K_tgt spread over them: what observed_reproject_cases.closed_form reads"""
    R, V = c["R"], c["V"]
    Hs, Ws = c["depth_src"].shape[2:]
    return dict(c, depth_src=c["depth_src"].reshape(R * V, Hs, Ws), labels_src=c["labels_src"].reshape(R * V, Hs, Ws), k_src=c["k_src"].reshape(R * V, 4),
                pose=c["pose"].reshape(R * V, 3, 4), K_tgt=c["K_tgt"].repeat_interleave(V, 0))


def torch_route(c, dtype):
    """``reproject_views_torch`` of a case with the rasterizer's C restatement, computed once per (case, dtype) and never modified"""
    return OC.torch_route(c, dtype, "reproject_views_torch")


def whole_route(c, dtype):
    """``reproject_torch`` of the uncut frame of split_plane_18x34_s32 through the same rasterizer, once per dtype"""
    return OC.torch_route(c["whole"], dtype)


def seam(face_index, Hs, Ws, cut):
    """[B, S, S] bool in the planes' row order: the pixels whose winning cell in a whole frame's ``face_index`` (raster order) has column
    ``cut - 1`` or ``cut`` - the cells on either side of the column both halves keep"""
    fi = face_index.long()
    Wc = Ws - 1
    col = (fi.clamp(min=0) // 2) % Wc
    hit = (fi >= 0) & (fi < 2 * (Hs - 1) * Wc)
    return torch.flip(hit & ((col == cut - 1) | (col == cut)), [1])


def plane_pixels(c, out):
    """For a fused result ``out`` (depth, source in the planes' row order, on the host) of a rasterized case: per frame b = r * V + v with a
    plane, (b, closed-form depth [S, S] float64, mask [S, S]) - mask: closed_form's ``inside`` pixels of that frame which frame v wins"""
    fr = frames(c)
    res = []
    for b, plane in enumerate(c["plane"]):
        if plane is None:
            continue
        r, v = divmod(b, c["V"])
        want, inside, _, _ = OC.closed_form(fr, b)
        res.append((b, want, inside & (out["source"][r] == v + 1)))
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# maps made by hand
# ------------------------------------------------------------------------------------------------------------------------------
MAPS_R, MAPS_V, MAPS_HS, MAPS_WS, MAPS_S = 2, 4, 5, 7, 33
MAPS_GAP = 0.05


def _agreement_edge(gap):
    """float32 (dmin, d_at, d_above): d_at - dmin == gap * dmin EXACTLY in float32 (so d_at still agrees), d_above one ulp further (so
    it does not).  Found by walking dmin upwards ulp by ulp from 1.5 until dmin + gap * dmin is a float32."""
    g, dmin = np.float32(gap), np.float32(1.5)
    for _ in range(100000):
        edge = g * dmin
        d_at = dmin + edge
        if np.float32(d_at - dmin) == edge and np.float64(dmin) + np.float64(edge) == np.float64(d_at):
            d_above = np.nextafter(d_at, np.float32(np.inf))
            assert np.float32(d_above - dmin) > edge and not np.float32(d_at - dmin) > edge
            return dmin, d_at, d_above
        dmin = np.nextafter(dmin, np.float32(np.inf))
    raise AssertionError("no exact edge found")


def _build_maps():
    R, V, Hs, Ws, S = MAPS_R, MAPS_V, MAPS_HS, MAPS_WS, MAPS_S
    B, F = R * V, 2 * (Hs - 1) * (Ws - 1)
    rng = np.random.default_rng(31)
    nan = float("nan")
    lab = torch.from_numpy(rng.integers(0, 256, (B, Hs, Ws)).astype(np.uint8))
    fi = torch.from_numpy(rng.integers(-1, F, size=(B, S, S)).astype(np.int32))
    w = torch.from_numpy(rng.dirichlet((1.0, 1.0, 1.0), size=(B, S, S)).astype(np.float32))
    dep = torch.from_numpy(rng.uniform(0.2, 9.0, (B, S, S)).astype(np.float32))
    # raster rows 8 .. 19 of room 0: depths on a grid of 0.25 (equal depths in two, three and four frames by chance), a sprinkle of
    # indices F and F + 1000, NaN weights and NaN depths
    dep[:V, 8:20] = torch.round(dep[:V, 8:20] * 4) / 4
    u = torch.from_numpy(rng.uniform(0, 1, (V, 12, S)))
    fi[:V, 8:20][u < 0.05] = F
    fi[:V, 8:20][(u >= 0.05) & (u < 0.1)] = F + 1000
    w[:V, 8:20][(u >= 0.1) & (u < 0.2)] = torch.tensor([0.5, nan, 0.5])
    dep[:V, 8:20][(u >= 0.2) & (u < 0.3)] = nan
    # raster row 0 of room 0 (the planes' row S - 1), pixel by pixel
    dmin, d_at, d_above = (float(x) for x in _agreement_edge(MAPS_GAP))
    fi[:V, 0, :8] = torch.tensor([3, 10, 21, F - 1], dtype=torch.int32)[:, None]
    w[:V, 0, :8] = torch.tensor([0.2, 0.3, 0.5])
    fi[:V, 0, 0] = torch.tensor([-1, F, F + 1000, -1], dtype=torch.int32)        # 0: no frame hits
    dep[:V, 0, 1] = torch.tensor([3.0, 1.0, 2.0, 4.0]); w[1, 0, 1] = torch.tensor([nan, 0.5, 0.5])       # 1: NaN weights on the nearest
    dep[:V, 0, 2] = torch.tensor([nan, 5.0, 6.0, 7.0])                            # 2: a NaN depth on a hit
    dep[:V, 0, 3] = torch.tensor([4.0, 2.5, 2.5, 3.0])                            # 3: equal depths in two frames
    dep[:V, 0, 4] = torch.tensor([1.5, 1.5, 9.0, 1.5])                            # 4: equal depths in three
    dep[:V, 0, 5] = torch.tensor([dmin, d_at, d_above, 2 * dmin])                 # 5: the agreement edge
    dep[:V, 0, 6] = torch.tensor([4.0, 3.0, 2.0, 1.0])                            # 6: every frame nearer than the one before
    dep[:V, 0, 7] = torch.tensor([2.0, 1.0, 1.0, 1.0]); w[1, 0, 7] = torch.tensor([0.5, 0.5, nan]); w[2, 0, 7] = torch.tensor([0.1, 0.2, 0.7])   # 7: both
    # room 1: every frame misses everywhere
    fi[V:] = torch.from_numpy(rng.choice(np.array([-1, F, F + 1000, -7], dtype=np.int32), size=(V, S, S)))
    return dict(R=R, V=V, Hs=Hs, Ws=Ws, S=S, F=F, gap=MAPS_GAP, face_index=fi, weight=w, raster_depth=dep, labels_src=lab,
                edge=(dmin, d_at, d_above))


def maps():
    if "maps" not in _CACHE:
        _CACHE["maps"] = _build_maps()
    return _CACHE["maps"]


def junk(R, V, S, device="cpu"):
    """the seven outputs, pre-filled with values no result holds"""
    return OC.junk(dict(depth=(R, S, S), labels=(R, S, S), source=(R, S, S), count=(R, S, S), agree=(R, S, S), hits=(R,), wins=(R, V)), device)
