"""Fusion of several observed frames per room on the device (csrc/observed_fuse.hip through host/reproject.py; run with -m gpu): the
fused compose exactly against ``fuse_torch`` on the rasterizer's C restatement run on the device's own faces, the bare entry point on
hand-made maps with and without its optional outputs, V = 1 against ``ObservedReprojector``, planes against their closed form, the same
bytes from call to call and under graph replays, the refusals, and the round trip of a device render cut in two into
``RefineBatch(observed=, mask=)``."""
import ctypes as C

import numpy as np
import pytest
import torch

import observed_fuse_cases as FC
import observed_reproject_cases as OC
from conftest import pkg
from gpu_util import _lib, _sync

pytestmark = pytest.mark.gpu

# Largest |depth - closed form of the winner's plane| of the float32 torch route with the C rasterizer over the fused plane cases, on the
# pixels closed_form calls inside and the plane's frame wins: measured 2.661e-06 (tests/test_observed_fuse_host.py prints it per frame and
# holds this constant to at most 10 % above it).  The device route - FMA contraction, another order - is allowed four times that, as in
# test_observed_reproject_gpu.py.
FUSE_PLANE_F32_ERR = 2.8e-6

OUT = ("depth", "labels", "source", "count", "agree", "hits", "wins")


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def _inputs(c):
    return tuple(c[k].cuda() for k in ("depth_src", "labels_src", "k_src", "pose", "K_tgt")) + (c["orig_size"],)


def _fuser(c):
    RP = pkg("host.reproject")
    Hs, Ws = c["depth_src"].shape[2:]
    return RP.ObservedFuser(Hs, Ws, c["S"], rooms=c["R"], views=c["V"], near=c["near"], far=c["far"], gap=c["gap"])


def _run(c):
    fu = _fuser(c)
    fu(*_inputs(c))
    _sync("ObservedFuser %s" % c["name"])
    return fu


def _outputs(fu):
    return {k: getattr(fu, k) for k in OUT}


@pytest.mark.parametrize("name", FC.NAMES)
def test_fused_compose_exactly_against_the_torch_definition(name):
    """G1"""
    from oracle import raster_ref
    _lib()
    RP = pkg("host.reproject")
    c = FC.case(name)
    fu = _run(c)
    fx = fu.faces_xyz.cpu()
    fi, w, dep = (torch.from_numpy(x) for x in raster_ref.nmr_forward(fx.numpy(), c["S"], c["near"], c["far"]))
    assert torch.equal(fu.face_index.cpu(), fi) and torch.equal(_bits(fu.weight.cpu()), _bits(w)) and torch.equal(_bits(fu.raster_depth.cpu()), _bits(dep))
    lab = c["labels_src"].reshape(c["R"] * c["V"], *c["labels_src"].shape[2:])
    want = RP.fuse_torch(fi, w, dep, lab, c["V"], c["gap"])
    got = _outputs(fu)
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and _same(got[k].cpu(), want[k]), k
    assert got["depth"].dtype == torch.float32 and got["hits"].dtype == torch.int64 and got["wins"].dtype == torch.int64
    assert all(got[k].dtype == torch.uint8 for k in ("labels", "source", "count", "agree"))
    assert torch.equal(got["wins"].sum(1), got["hits"]) and torch.equal(fu.valid().cpu(), (want["source"] > 0).to(torch.uint8))
    if name == "nothing_3x5_s16":
        assert int(got["hits"].sum()) == 0 and bool((got["depth"] == -1).all())
    else:
        assert int(got["hits"][0]) * 4 >= c["S"] ** 2


def test_bare_entry_point_on_hand_made_maps_with_and_without_the_optional_outputs():
    """G2"""
    _lib()
    RP = pkg("host.reproject")
    m = FC.maps()
    R, V, S = m["R"], m["V"], m["S"]
    want = RP.fuse_torch(m["face_index"], m["weight"], m["raster_depth"], m["labels_src"], V, m["gap"])
    maps = [m[k].cuda() for k in ("face_index", "weight", "raster_depth", "labels_src")]
    out = FC.junk(R, V, S, "cuda")
    RP.fuse(*maps, V, m["gap"], out["depth"], out["labels"], out["hits"], out["source"], out["count"], out["agree"], out["wins"])
    _sync("sln_reproject_fuse on hand-made maps")
    for k in OUT:
        assert _same(out[k].cpu(), want[k]), k
    assert out["source"][0, S - 1, :8].tolist() == [0, 3, 2, 2, 1, 1, 4, 3] and out["agree"][0, S - 1, :8].tolist() == [0, 1, 1, 2, 3, 2, 1, 2]
    # without the optional outputs: they stay untouched, the required ones are the same
    again, fresh = FC.junk(R, V, S, "cuda"), FC.junk(R, V, S)
    RP.fuse(*maps, V, m["gap"], again["depth"], again["labels"], again["hits"])
    _sync("sln_reproject_fuse without the optional outputs")
    for k in ("depth", "labels", "hits"):
        assert _same(again[k].cpu(), want[k]), k
    for k in ("source", "count", "agree", "wins"):
        assert torch.equal(again[k].cpu(), fresh[k]), k


def test_one_view_equals_the_reprojector():
    """G3"""
    _lib()
    RP = pkg("host.reproject")
    c = FC.case("one_view_48x64_s64")
    fu = _run(c)
    d, l, k, P, K, orig = _inputs(c)
    Hs, Ws = c["depth_src"].shape[2:]
    rp = RP.ObservedReprojector(Hs, Ws, c["S"], batch=c["R"], near=c["near"], far=c["far"], gap=c["gap"])
    depth, labels, hits = rp(d[:, 0].contiguous(), l[:, 0].contiguous(), k[:, 0].contiguous(), P[:, 0].contiguous(), K, orig)
    _sync("ObservedReprojector on the same frames")
    assert torch.equal(_bits(fu.depth), _bits(depth)) and torch.equal(fu.labels, labels) and torch.equal(fu.hits, hits)
    assert int(hits[0]) > 0 and int(hits[2]) > 0 and torch.equal(fu.wins[:, 0], hits)


def test_fused_planes_end_to_end_against_the_closed_form():
    """G4: on the host test's pixel set, within four times the float32 torch route's figure"""
    _lib()
    checked = 0
    for c in FC.cases():
        fu = _run(c)
        out = {k: v.cpu() for k, v in _outputs(fu).items()}
        for b, want, m in FC.plane_pixels(c, out):
            if bool(m.any()):
                err = float((out["depth"][b // c["V"]].double() - want)[m].abs().max())
                print("%s frame %d: device route against the closed form on %d pixels: %.3e (allowed %.3e)" % (c["name"], b, int(m.sum()), err, 4 * FUSE_PLANE_F32_ERR))
                assert err <= 4.0 * FUSE_PLANE_F32_ERR
                checked += int(m.sum())
    assert checked >= 1000


def test_same_bytes_from_call_to_call_and_under_graph_replays():
    """G5"""
    L = _lib()
    c = FC.case("two_rooms_18x34_s32")
    args = _inputs(c)
    fu = _fuser(c)
    junk = FC.junk(c["R"], c["V"], c["S"], "cuda")

    def refill():
        for k in OUT:
            getattr(fu, k).copy_(junk[k])
    firsts = []
    try:
        for det in (0, 1):
            L.lib().sln_set_deterministic(det)
            refill()
            fu(*args)
            _sync("first call")
            first = {k: v.clone() for k, v in _outputs(fu).items()}
            refill()
            fu(*args)
            _sync("second call")
            assert all(_same(first[k], getattr(fu, k)) for k in OUT)
            firsts.append(first)
    finally:
        L.lib().sln_set_deterministic(0)
    assert all(_same(firsts[0][k], firsts[1][k]) for k in OUT), "either deterministic setting"
    first = firsts[0]
    assert int(first["hits"][0]) > 0 and int(first["hits"][1]) > 0 and not torch.equal(first["depth"][0], first["depth"][1])
    args = tuple(a.clone() if torch.is_tensor(a) else a for a in args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fu(*args)
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fu(*args)
    for _ in range(2):
        refill()
        graph.replay()
        _sync("replay of the fusion")
        assert all(_same(first[k], getattr(fu, k)) for k in OUT)
    # other contents through the same graph: the rooms change places, with their cameras
    for a in args[:5]:
        a.copy_(a[[1, 0]].clone())
    refill()
    graph.replay()
    _sync("replay with the rooms swapped")
    assert all(_same(first[k][[1, 0]], getattr(fu, k)) for k in OUT)


def test_refusals_leave_the_outputs_untouched():
    """G6"""
    L = _lib()
    RP = pkg("host.reproject")
    c = FC.case("near_wins_18x34_s32")
    R, V, S = c["R"], c["V"], c["S"]
    Hs, Ws = c["depth_src"].shape[2:]
    fu = _run(c)
    first = {k: v.clone() for k, v in _outputs(fu).items()}
    junk = FC.junk(R, V, S, "cuda")
    for k in OUT:
        getattr(fu, k).copy_(junk[k])
    d, l, k, P, K, orig = _inputs(c)
    bad = [(d.cpu(), l, k, P, K, orig), (d.double(), l, k, P, K, orig), (d, l.to(torch.int32), k, P, K, orig), (d[:, :, :2].contiguous(), l, k, P, K, orig),
           (d.reshape(R * V, Hs, Ws), l, k, P, K, orig), (d, l, k[..., :3].contiguous(), P, K, orig), (d, l, k, P[..., :3].contiguous(), K, orig),
           (d, l, k, P, K.cpu(), orig), (d, l, k, P, K.repeat_interleave(V, 0), orig), (d, l, k, P.transpose(2, 3).contiguous().transpose(2, 3), K, orig),
           (d, l, k, P, K, 0.0), (d, l, k, P, K, float("nan"))]
    for args in bad:
        with pytest.raises(ValueError):
            fu(*args)
    lib, ptr, st = L.lib(), L.ptr, L.current_stream_ptr()
    lab = l.view(R * V, Hs, Ws)

    def call(R_=R, V_=V, Hs_=Hs, Ws_=Ws, S_=S, gap=c["gap"], null=None, **at):
        a = [ptr(fu.face_index), ptr(fu.weight), ptr(fu.raster_depth), ptr(lab), R_, V_, Hs_, Ws_, S_, gap, ptr(fu.depth), ptr(fu.labels), ptr(fu.source),
             ptr(fu.count), ptr(fu.agree), ptr(fu.hits), ptr(fu.wins), st]
        if null is not None:
            a[null] = None
        for i, v in at.items():
            a[int(i[1:])] = v
        return lib.sln_reproject_fuse(*a)
    for kw in (dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=10), dict(null=11), dict(null=15), dict(R_=0), dict(V_=0), dict(V_=256),
               dict(R_=258, V_=255), dict(Hs_=1), dict(Ws_=1), dict(S_=0), dict(S_=4097), dict(Hs_=4097, Ws_=2050), dict(gap=-0.01), dict(gap=float("nan")),
               dict(a15=C.c_void_p(fu.hits.data_ptr() + 4)), dict(a16=C.c_void_p(fu.wins.data_ptr() + 4)), dict(a10=C.c_void_p(fu.depth.data_ptr() + 2))):
        assert call(**kw) == -1, kw
    _sync("refused calls")
    for k_ in OUT:
        assert torch.equal(getattr(fu, k_), junk[k_]), k_
    fu(d, l, k, P, K, orig)                                          # ... and the same call with nothing wrong goes through
    _sync("the sound call")
    assert int(first["hits"][0]) > 0 and all(_same(first[k_], getattr(fu, k_)) for k_ in OUT)


def test_round_trip_of_a_device_render_cut_in_two_into_refine_batch():
    """G7: the room of test_observed_reproject_gpu's T5 rendered at S = 64, observed, and cut into two overlapping halves at column 32
    (frame 0 keeps the columns <= 32, frame 1 the columns >= 32) beside a third frame with fx = 0; identity poses, scene_as_source.  On
    the settled pixels outside the seam set (the pixels whose winning cell in the whole frame has column 31 or 32: three columns of 64 by
    the identity geometry) there is a winner, the label is the source's and depth is within four times the float32 route's figure for
    this room.  RefineBatch(observed=, mask=fuser.valid()) takes the pair and runs an iteration."""
    from test_observed_reproject_gpu import ROUND_TRIP_F32_ERR, _round_trip_room
    _lib()
    RP, OB, R = pkg("host.reproject"), pkg("host.observe"), pkg("host.refine")
    cfg, rooms, bank, room_model = _round_trip_room()
    rm, S, cut = rooms[0], OC.ROUND_TRIP_S, 32
    with torch.no_grad():
        render = R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), S).render(rm["boxes"], rm["angles"].float())[0]
    src_depth, src_labels = OB.observe(render)
    k_src, pose, K, orig = OC.round_trip_inputs(rm["boxes"][-1], S, B=3)
    k_src[2, 0] = 0.0                                                # the padding frame
    depth_v, labels_v = src_depth.repeat(3, 1, 1), src_labels.repeat(3, 1, 1)
    depth_v[0, :, cut + 1:] = 0.0; labels_v[0, :, cut + 1:] = 0
    depth_v[1, :, :cut] = 0.0; labels_v[1, :, :cut] = 0
    fu = RP.ObservedFuser(S, S, S, rooms=1, views=3)
    depth, labels, source = fu(depth_v[None].contiguous(), labels_v[None].contiguous(), k_src[None].cuda(), pose[None].cuda(), K[:1].cuda(), orig)
    _sync("fusion of the two halves of a device render")
    rp = RP.ObservedReprojector(S, S, S, batch=1)
    rp(src_depth, src_labels, k_src[:1].cuda(), pose[:1].cuda(), K[:1].cuda(), orig)
    _sync("the whole frame")
    seam = FC.seam(rp.face_index, S, S, cut)
    ok = OC.settled(src_depth.cpu(), src_labels.cpu()).cuda() & ~seam
    won = source > 0
    err = float((depth - src_depth)[ok & won].abs().max())
    print("round trip of two halves: %d settled pixels outside the seam of %d (seam %d), %d winners, without a winner %d, another label %d, "
          "largest depth error %.3e (allowed %.3e); wins %s" % (int(ok.sum()), S * S, int(seam.sum()), int(fu.hits[0]), int((ok & ~won).sum()),
                                                                 int((ok & (labels != src_labels)).sum()), err, 4 * ROUND_TRIP_F32_ERR, fu.wins.tolist()))
    assert 2 * int(OC.settled(src_depth.cpu(), src_labels.cpu()).sum()) >= S * S and 10 * int(seam.sum()) <= S * S
    assert not bool((ok & ~won).any()) and torch.equal(labels[ok], src_labels[ok]) and err <= 4.0 * ROUND_TRIP_F32_ERR
    assert int(fu.wins[0, 0]) > 0 and int(fu.wins[0, 1]) > 0 and int(fu.wins[0, 2]) == 0 and int(fu.hits[0]) == int(won.sum())
    model, _ = room_model(cfg)
    rb = R.RefineBatch(model, rooms, observed=(depth, labels), mask=fu.valid(), bank=bank, learning_rate=1e-3, image_size=S, iters=1)
    try:
        losses = rb.run().cpu().numpy().copy()
        _sync("one iteration towards the fused pair")
        status = rb.target_status.tolist()
    finally:
        rb.close()
    assert np.isfinite(losses).all() and losses.shape[0] == 1
    assert status[0] & OB.STATUS_NO_WALL == 0, "the wall bit of target_status is clear"
