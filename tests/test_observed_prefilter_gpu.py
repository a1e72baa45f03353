"""Pre-filter of observed frames finer than the target on the device (csrc/observed_prefilter.hip through host/reproject.py; run with
-m gpu): the kernel exactly against ``prefilter_torch`` on every hand-made case with sentinels behind every output, with and without
``counts``, the same bytes from call to call and under graph replays, ``ObservedReprojector(prefilter=)`` and ``ObservedFuser(prefilter=)``
against the unfiltered instances on ``ObservedPrefilter``'s outputs, ``prefilter=1`` against the instance built without the keyword,
planes through the whole device route against their closed form, and one ``RefineBatch(observed=, mask="readings")`` iteration on a
filtered pair."""
import numpy as np
import pytest
import torch

import observed_prefilter_cases as PC
import observed_reproject_cases as OC
from conftest import load_golden, pkg
from gpu_util import _lib, _sync

pytestmark = pytest.mark.gpu

# Largest |depth - closed form| of the float32 torch route with the C rasterizer on the FILTERED plane frames of
# observed_prefilter_cases (f = 2, 4 and 8), on the target pixels whose source position lies a full coarse pixel inside the coarse grid:
# measured 1.174e-06 (tests/test_observed_prefilter_host.py prints it per frame and holds this constant to at most twice the worst).
# The device route - FMA contraction, another order - is allowed four times that, as in test_observed_reproject_gpu.py.
PREFILTER_PLANE_F32_ERR = 1.25e-6

OUT = ("depth", "labels", "k_out", "counts")
PAD = 67                                                             # sentinel elements behind every output


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float32 else torch.equal(a, b)


def _padded(c):
    """the four outputs as views of buffers that go on for PAD sentinel elements -> (views, whole buffers, sizes)"""
    B, Hs, Ws = c["depth_src"].shape
    Hd, Wd = Hs // c["f"], Ws // c["f"]
    shapes = dict(depth=(B, Hd, Wd), labels=(B, Hd, Wd), k_out=(B, 4), counts=(B, 3))
    junk = PC.junk(1, 1, 1)
    whole = {k: torch.full((int(np.prod(shapes[k])) + PAD,), junk[k].flatten()[0].item(), dtype=junk[k].dtype, device="cuda") for k in OUT}
    views = {k: whole[k][:int(np.prod(shapes[k]))].view(shapes[k]) for k in OUT}
    return views, whole, junk


def _tails_untouched(whole, junk):
    return all(bool((whole[k][-PAD:] == junk[k].flatten()[0].item()).all()) for k in OUT)


@pytest.mark.parametrize("name", PC.NAMES)
def test_kernel_exactly_against_the_torch_definition(name):
    """G1 and G2: depth bits, label bytes, k_out bits and counts; sentinels behind every output; without counts nothing else changes"""
    _lib()
    RP = pkg("host.reproject")
    c = PC.case(name)
    want = dict(zip(OUT, PC.filtered(c)))
    src = [c[k].cuda() for k in ("depth_src", "labels_src", "k_src")]
    out, whole, junk = _padded(c)
    RP.prefilter(*src, c["f"], c["gap"], out["depth"], out["labels"], out["k_out"], out["counts"])
    _sync("sln_observed_prefilter %s" % name)
    for k in OUT:
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape and _same(out[k].cpu(), want[k]), k
    assert _tails_untouched(whole, junk)
    again, whole2, _ = _padded(c)
    RP.prefilter(*src, c["f"], c["gap"], again["depth"], again["labels"], again["k_out"])
    _sync("sln_observed_prefilter %s without counts" % name)
    assert all(_same(again[k], out[k]) for k in ("depth", "labels", "k_out")) and _tails_untouched(whole2, junk)
    assert bool((whole2["counts"] == -3).all()), "counts = NULL: nothing written there"


def test_same_bytes_from_call_to_call_and_under_graph_replays():
    """G3"""
    L = _lib()
    RP = pkg("host.reproject")
    c = PC.case("holes_37x70_f2")
    B, Hs, Ws = c["depth_src"].shape
    src = [c[k].cuda() for k in ("depth_src", "labels_src", "k_src")]
    pf = RP.ObservedPrefilter(Hs, Ws, c["f"], batch=B, gap=c["gap"])
    junk = PC.junk(B, pf.Hd, pf.Wd, "cuda")

    def refill():
        for k in OUT:
            getattr(pf, k).copy_(junk[k])
    firsts = []
    try:
        for det in (0, 1):
            L.lib().sln_set_deterministic(det)
            refill()
            got = pf(*src)
            _sync("first call")
            assert got[0] is pf.depth and got[1] is pf.labels and got[2] is pf.k_out
            first = {k: getattr(pf, k).clone() for k in OUT}
            refill()
            pf(*src)
            _sync("second call")
            assert all(_same(first[k], getattr(pf, k)) for k in OUT)
            firsts.append(first)
    finally:
        L.lib().sln_set_deterministic(0)
    assert all(_same(firsts[0][k], firsts[1][k]) for k in OUT), "either deterministic setting"
    first = firsts[0]
    assert all(_same(first[k].cpu(), w) for k, w in zip(OUT, PC.filtered(c)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pf(*src)
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pf(*src)
    for _ in range(2):
        refill()
        graph.replay()
        _sync("replay of the pre-filter")
        assert all(_same(first[k], getattr(pf, k)) for k in OUT)
    # the instance refuses what is not its frames before anything is launched
    refill()
    d, l, k = src
    for args in ((d.cpu(), l, k), (d.double(), l, k), (d, l.to(torch.int32), k), (d[:, :4].contiguous(), l, k), (d, l, k[:, :3].contiguous())):
        with pytest.raises(ValueError):
            pf(*args)
    _sync("refused calls")
    assert all(torch.equal(getattr(pf, k_), junk[k_]) for k_ in OUT)


def _inputs(c):
    return tuple(c[k].cuda() for k in ("depth_src", "labels_src", "k_src", "pose", "K_tgt")) + (c["orig_size"],)


def _reprojector(c, Hs, Ws, **kw):
    return pkg("host.reproject").ObservedReprojector(Hs, Ws, c["S"], batch=c["depth_src"].shape[0], near=c["near"], far=c["far"], gap=c["gap"], **kw)


@pytest.mark.parametrize("name", ["plane_37x70_f2", "frames_48x64_f4", "speckles_16x24_f8"])
def test_reprojector_with_the_keyword_equals_the_reprojector_on_the_filtered_frames(name):
    """G4"""
    _lib()
    RP = pkg("host.reproject")
    c = PC.case(name)
    B, Hs, Ws = c["depth_src"].shape
    d, l, k, P, K, orig = _inputs(c)
    rp = _reprojector(c, Hs, Ws, prefilter=c["f"])
    rp(d, l, k, P, K, orig)
    _sync("ObservedReprojector(prefilter=%d) %s" % (c["f"], name))
    pf = RP.ObservedPrefilter(Hs, Ws, c["f"], batch=B, gap=c["gap"])
    cd, cl, ck = pf(d, l, k)
    plain = _reprojector(c, pf.Hd, pf.Wd)
    plain(cd, cl, ck, P, K, orig)
    _sync("ObservedReprojector on ObservedPrefilter's outputs")
    assert rp.F == plain.F == 2 * (pf.Hd - 1) * (pf.Wd - 1) and rp.faces_xyz.shape == plain.faces_xyz.shape
    assert all(_same(getattr(rp, a), getattr(plain, a)) for a in ("depth", "labels", "hits", "faces_xyz", "face_index", "raster_depth"))
    assert all(_same(getattr(rp.pre, a), getattr(pf, a)) for a in OUT)
    assert all(_same(getattr(pf, a).cpu(), w) for a, w in zip(OUT, PC.filtered(c)))
    assert int(rp.hits.sum()) > 0


def test_fuser_with_the_keyword_equals_the_fuser_on_the_filtered_frames():
    """G5: R = 2, V = 2 out of the frames of frames_48x64_f4, the rooms' K_tgt those of frames 0 and 2"""
    _lib()
    RP = pkg("host.reproject")
    c = PC.case("frames_48x64_f4")
    R, V, f = 2, 2, c["f"]
    Hs, Ws = c["depth_src"].shape[1:]
    pick = [0, 1, 2, 0]
    d, l, k, P = (c[a][pick].reshape(R, V, *c[a].shape[1:]).contiguous().cuda() for a in ("depth_src", "labels_src", "k_src", "pose"))
    K = c["K_tgt"][[0, 2]].contiguous().cuda()
    kw = dict(rooms=R, views=V, near=c["near"], far=c["far"], gap=c["gap"])
    fu = RP.ObservedFuser(Hs, Ws, c["S"], prefilter=f, **kw)
    fu(d, l, k, P, K, c["orig_size"])
    _sync("ObservedFuser(prefilter=%d)" % f)
    pf = RP.ObservedPrefilter(Hs, Ws, f, batch=R * V, gap=c["gap"])
    cd, cl, ck = pf(d.view(R * V, Hs, Ws), l.view(R * V, Hs, Ws), k.view(R * V, 4))
    plain = RP.ObservedFuser(pf.Hd, pf.Wd, c["S"], **kw)
    plain(cd.view(R, V, pf.Hd, pf.Wd), cl.view(R, V, pf.Hd, pf.Wd), ck.view(R, V, 4), P, K, c["orig_size"])
    _sync("ObservedFuser on ObservedPrefilter's outputs")
    for a in ("depth", "labels", "source", "count", "agree", "hits", "wins", "faces_xyz"):
        assert _same(getattr(fu, a), getattr(plain, a)), a
    assert all(int(x) > 0 for x in fu.hits) and int((fu.count >= 2).sum()) > 0


def test_prefilter_one_is_the_instance_without_the_keyword():
    """G6: the default runs no filter - non-readings reach the face kernel as they are - and owns no filter"""
    _lib()
    RP = pkg("host.reproject")
    c = OC.case("tile_edge_18x34_s32")
    B, Hs, Ws = c["depth_src"].shape
    args = _inputs(c)
    a, b = _reprojector(c, Hs, Ws), _reprojector(c, Hs, Ws, prefilter=1)
    a(*args); b(*args)
    _sync("ObservedReprojector with and without prefilter=1")
    assert b.pre is None and a.pre is None and a.F == b.F == RP.n_faces(Hs, Ws)
    assert all(_same(getattr(a, x), getattr(b, x)) for x in ("depth", "labels", "hits", "faces_xyz", "face_index", "weight", "raster_depth"))
    assert int(a.hits.sum()) > 0
    d, l, k, P, K, orig = args
    kw = dict(rooms=1, views=B, near=c["near"], far=c["far"], gap=c["gap"])
    fa, fb = RP.ObservedFuser(Hs, Ws, c["S"], **kw), RP.ObservedFuser(Hs, Ws, c["S"], prefilter=1, **kw)
    for fu in (fa, fb):
        fu(d[None], l[None], k[None], P[None], K[:1].contiguous(), orig)
    _sync("ObservedFuser with and without prefilter=1")
    assert fb.pre is None and all(_same(getattr(fa, x), getattr(fb, x)) for x in ("depth", "labels", "source", "count", "agree", "hits", "wins", "faces_xyz"))


def test_filtered_planes_end_to_end_against_the_closed_form():
    """G7: on the host test's pixel set, within four times the float32 torch route's figure"""
    _lib()
    checked = 0
    for name in PC.ROUTE_NAMES:
        c = PC.case(name)
        Hs, Ws = c["depth_src"].shape[1:]
        rp = _reprojector(c, Hs, Ws, prefilter=c["f"])
        depth, labels, hits = rp(*_inputs(c))
        _sync("ObservedReprojector(prefilter=%d) %s" % (c["f"], name))
        depth = depth.cpu()
        for b, plane in enumerate(c["plane"]):
            if plane is None:
                continue
            want, inside, _, _ = OC.closed_form(PC.coarse(c), b)
            assert not bool((inside & ~(depth[b] > 0)).any()), "a plane is hit on every inside pixel"
            err = float((depth[b].double() - want)[inside].abs().max())
            print("%s frame %d (f = %d): device route against the closed form on %d pixels: %.3e (allowed %.3e)" % (
                name, b, c["f"], int(inside.sum()), err, 4 * PREFILTER_PLANE_F32_ERR))
            assert err <= 4.0 * PREFILTER_PLANE_F32_ERR
            checked += int(inside.sum())
    assert checked >= 300


def test_one_refine_batch_iteration_on_a_filtered_pair():
    """G8: the recorded observation of the round-trip room (tests/golden/observed_reproject_room.npz, 64 x 64) filtered at f = 2 and
    brought into the room's own view at S = 64: the pair goes into RefineBatch(observed=, mask="readings") and an iteration runs.
    (The frame is no finer than the view - prefilter_factor says 1 - and its lens is wide, 25 pixels of focal length on 64: at half the
    resolution most cells of the floor and the walls exceed the depth step and are cut, so few pixels are hit.  The test is about the
    plumbing: whatever was hit carries a label of the frame, the rest reads "no reading" and the mask keeps it out of the loss.)"""
    from test_observed_reproject_gpu import _round_trip_room
    _lib()
    RP, OB, R = pkg("host.reproject"), pkg("host.observe"), pkg("host.refine")
    g = load_golden("observed_reproject_room")
    S = OC.ROUND_TRIP_S
    src_depth, src_labels = torch.from_numpy(g["depth"]).cuda(), torch.from_numpy(g["labels"]).cuda()
    cfg, rooms, bank, room_model = _round_trip_room()
    k_src, pose, K, orig = OC.round_trip_inputs(g["room"], S)
    assert RP.prefilter_factor(k_src, K, orig, S) == 1, "the frame is as fine as the view: the caller passes the larger factor"
    rp = RP.ObservedReprojector(S, S, S, batch=1, prefilter=2)
    depth, labels, hits = rp(src_depth, src_labels, k_src.cuda(), pose.cuda(), K.cuda(), orig)
    _sync("the filtered round trip")
    assert rp.pre.counts.sum().item() == (S // 2) ** 2 and rp.F == 2 * (S // 2 - 1) ** 2
    assert int(hits[0]) == int((depth > 0).sum()) > 0 and torch.equal(depth == -1, ~(depth > 0)) and bool((labels[depth == -1] == 0).all())
    seen = set(labels[depth > 0].tolist())
    assert seen and seen <= set(src_labels.flatten().tolist()), "no label the frame does not hold"
    model, _ = room_model(cfg)
    rb = R.RefineBatch(model, rooms, observed=(depth, labels), mask="readings", bank=bank, learning_rate=1e-3, image_size=S, iters=1)
    try:
        losses = rb.run().cpu().numpy().copy()
        _sync("one iteration towards the filtered pair")
        status = rb.target_status.tolist()
    finally:
        rb.close()
    assert np.isfinite(losses).all() and losses.shape[0] == 1
    assert status[0] & OB.STATUS_NO_WALL == 0, "the wall bit of target_status is clear"
