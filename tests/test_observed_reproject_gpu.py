"""Reprojection of observed frames on the device (csrc/observed_reproject.hip through host/reproject.py; run with -m gpu), at operand
level: the face kernel against the float64 restatement, the compose kernel exactly against the torch compose on the rasterizer's C
restatement run on the device's own faces, hand-made maps, planes against their closed form, the round trip of a device render into
``RefineBatch(observed=)``, repeatability and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import observed_reproject_cases as OC
from conftest import pkg
from gpu_util import _lib, _sync

pytestmark = pytest.mark.gpu

# (i) Largest |fp32 - fp64| / max(1, |fp64|) over the kept slots of every case of observed_reproject_cases, with both restatements run in
# torch on the host: measured 3.327e-07 (tests/test_observed_reproject_host.py prints it per case and holds this constant to it).  The
# kernel does the same operations with FMA contraction and in another order - its only licence - and is allowed four times that figure.
FP32_TORCH_ERR = 3.4e-7
KERNEL_ALLOWANCE = 4.0 * FP32_TORCH_ERR
# (ii) Largest |depth - closed form| of the float32 torch route with the C rasterizer over the plane frames, on the target pixels whose
# source position lies a full source pixel inside the grid: measured 2.661e-06 (same host test file).
PLANE_F32_ERR = 2.8e-6
# The same route on the recorded render of the round-trip room (tests/golden/observed_reproject_room.npz), largest |depth - source depth|
# over the settled pixels: measured 2.027e-06.
ROUND_TRIP_F32_ERR = 2.1e-6


def _bits(a):
    return a.contiguous().view(torch.int32)


def _inputs(c):
    return tuple(c[k].cuda() for k in ("depth_src", "labels_src", "k_src", "pose", "K_tgt")) + (c["orig_size"],)


def _run(c):
    RP = pkg("host.reproject")
    B, Hs, Ws = c["depth_src"].shape
    rp = RP.ObservedReprojector(Hs, Ws, c["S"], batch=B, near=c["near"], far=c["far"], gap=c["gap"])
    out = rp(*_inputs(c))
    _sync("ObservedReprojector %d frames of %dx%d at %d" % (B, Hs, Ws, c["S"]))
    return rp, out


@pytest.mark.parametrize("name", OC.NAMES)
def test_faces_against_fp64_and_compose_exactly(name):
    """T1 and T2"""
    from oracle import raster_ref
    _lib()
    RP = pkg("host.reproject")
    c = OC.case(name)
    rp, (depth, labels, hits) = _run(c)
    want = OC.torch_route(c, torch.float64)
    fx = rp.faces_xyz.cpu()
    assert fx.shape == want["faces_xyz"].shape
    err, flips = OC.face_error(fx, want["faces_xyz"])
    print("%s: kernel against fp64, largest |d| / max(1, |want|) = %.3e (allowed %.3e; fp32 torch %.3e)" % (name, err, KERNEL_ALLOWANCE, FP32_TORCH_ERR))
    assert flips == 0 and err <= KERNEL_ALLOWANCE
    # the rasterizer's C restatement on the device's own faces: the device maps equal it, and the compose equals the torch compose
    fi, w, dep = (torch.from_numpy(x) for x in raster_ref.nmr_forward(fx.numpy(), c["S"], c["near"], c["far"]))
    assert torch.equal(rp.face_index.cpu(), fi) and torch.equal(_bits(rp.weight.cpu()), _bits(w)) and torch.equal(_bits(rp.raster_depth.cpu()), _bits(dep))
    d_w, l_w, h_w = RP.compose_torch(fi, w, dep, c["labels_src"])
    assert torch.equal(_bits(depth.cpu()), _bits(d_w)) and torch.equal(labels.cpu(), l_w) and torch.equal(hits.cpu(), h_w)
    assert hits.dtype == torch.int64 and depth.dtype == torch.float32 and labels.dtype == torch.uint8
    for b, shows in enumerate(c["shows"]):
        if shows is True:
            assert 4 * int(hits[b]) >= c["S"] ** 2
        if shows is False:
            assert int(hits[b]) == 0 and bool((depth[b] == -1).all()) and bool((labels[b] == 0).all())


def test_compose_on_hand_made_maps():
    """T3: indices -1, F and F + 1000; ties between two and three corners; a NaN weight; the row flip; outputs pre-filled with junk"""
    _lib()
    RP = pkg("host.reproject")
    B, Hs, Ws, S = 3, 5, 7, 33
    F = RP.n_faces(Hs, Ws)
    rng = np.random.default_rng(8)
    lab = torch.from_numpy(rng.integers(0, 256, (B, Hs, Ws)).astype(np.uint8))
    fi = torch.from_numpy(rng.integers(-1, F, size=(B, S, S)).astype(np.int32))
    w = torch.from_numpy(rng.dirichlet((1.0, 1.0, 1.0), size=(B, S, S)).astype(np.float32))
    dep = torch.from_numpy(rng.uniform(0.2, 9.0, (B, S, S)).astype(np.float32))
    fi[0, 0, :3] = torch.tensor([-1, F, F + 1000], dtype=torch.int32)
    fi[0, 1, :6] = torch.tensor([0, 1, 2, 3, F - 1, F - 2], dtype=torch.int32)
    ties = torch.tensor([[0.4, 0.4, 0.2], [0.2, 0.4, 0.4], [0.4, 0.2, 0.4], [1 / 3, 1 / 3, 1 / 3], [0.0, 0.0, 0.0], [0.25, 0.5, 0.25]])
    w[0, 1, :6] = ties
    w[0, 2, :3] = torch.tensor([[float("nan"), 0.5, 0.5], [0.5, float("nan"), 0.5], [0.5, 0.5, float("nan")]])
    fi[0, 2, :3] = 4
    fi[1] = -1                                                       # a frame without a hit
    fi[2, S - 1] = 5; dep[2, S - 1] = 0.75; w[2, S - 1] = torch.tensor([0.1, 0.2, 0.7])
    out = dict(depth=torch.full((B, S, S), 7.5).cuda(), labels=torch.full((B, S, S), 9, dtype=torch.uint8).cuda(),
               hits=torch.full((B,), -3, dtype=torch.int64).cuda())
    RP.compose(fi.cuda(), w.cuda(), dep.cuda(), lab.cuda(), out["depth"], out["labels"], out["hits"])
    _sync("sln_reproject_compose on hand-made maps")
    d_w, l_w, h_w = RP.compose_torch(fi, w, dep, lab)
    assert torch.equal(_bits(out["depth"].cpu()), _bits(d_w)) and torch.equal(out["labels"].cpu(), l_w) and torch.equal(out["hits"].cpu(), h_w)
    # what the yardstick must say about these maps, spelled out
    got_l, got_d = out["labels"].cpu(), out["depth"].cpu()
    assert got_d[0, S - 1, :3].tolist() == [-1.0, -1.0, -1.0] and got_l[0, S - 1, :3].tolist() == [0, 0, 0]
    # raster row 1 is the planes' row S - 2: corners 0, 1, 0, 0, 0, 1 of the slots 0, 1, 2, 3, F - 1, F - 2
    Wc = Ws - 1
    cell = lambda k: ((k // 2) // Wc, (k // 2) % Wc)
    px = {(0, 0): (0, 0), (0, 1): (1, 0), (0, 2): (0, 1), (1, 0): (1, 1), (1, 1): (0, 1), (1, 2): (1, 0)}       # (which, corner) -> pixel in the cell
    for x, (k, corner) in enumerate(((0, 0), (1, 1), (2, 0), (3, 0), (F - 1, 0), (F - 2, 1))):
        ci, cj = cell(k)
        di, dj = px[(k % 2, corner)]
        assert int(got_l[0, S - 2, x]) == int(lab[0, ci + di, cj + dj]), (x, k, corner)
        assert got_d[0, S - 2, x] == dep[0, 1, x]
    assert got_d[0, S - 3, :3].tolist() == [-1.0, -1.0, -1.0] and got_l[0, S - 3, :3].tolist() == [0, 0, 0], "a NaN weight is no hit"
    assert int(out["hits"][1]) == 0 and bool((got_d[1] == -1).all()) and bool((got_l[1] == 0).all())
    assert bool((got_d[2, 0] == 0.75).all()) and bool((got_l[2, 0] == lab[2, 1, 2]).all())      # slot 5 = (d, c, b) of cell (0, 2), corner 2 = b
    assert int(out["hits"][0]) == int(((fi[0] >= 0) & (fi[0] < F)).sum()) - 3


def test_planes_end_to_end_against_the_closed_form():
    """T4: on the host test's pixel set, within four times the float32 torch route's figure"""
    _lib()
    checked = 0
    for c in OC.cases():
        frames = [b for b in range(len(c["plane"])) if c["plane"][b] is not None and c["shows"][b] is not False]
        if not frames:
            continue
        rp, (depth, labels, hits) = _run(c)
        w64 = OC.torch_route(c, torch.float64)
        for b in frames:
            want, inside, _, _ = OC.closed_form(c, b)
            hit = depth[b].cpu() > 0
            if bool((~(w64["faces_xyz"][b] == 0).all(-1).all(-1)).all()):
                assert not bool((inside & ~hit).any()), "a frame without a hole is hit on every inside pixel"
            m = inside & hit
            if bool(m.any()):
                err = float((depth[b].cpu().double() - want)[m].abs().max())
                print("%s frame %d: device route against the closed form on %d pixels: %.3e (allowed %.3e)" % (c["name"], b, int(m.sum()), err, 4 * PLANE_F32_ERR))
                assert err <= 4.0 * PLANE_F32_ERR
                checked += int(m.sum())
    assert checked > 5000


def _round_trip_room():
    from oracle import vae_ref
    from test_refine_gpu import FURN, _random_rooms, _room_model
    R = pkg("host.refine")
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch", use_attr=False)
    rooms = _random_rooms(1, cfg, seed=OC.ROUND_TRIP_SEED)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    return cfg, rooms, bank, _room_model


def test_round_trip_of_a_device_render_into_refine_batch():
    """T5: a furnished RefineScene rendered at S = 64, observed, and reprojected with scene_as_source and the identity pose.  On every
    settled pixel (observed_reproject_cases.settled: at least half the image) there is a hit, the label is the source's and depth is
    within four times the float32 route's figure for this room.  RefineBatch(observed=) takes the pair and runs an iteration."""
    _lib()
    RP, OB, R = pkg("host.reproject"), pkg("host.observe"), pkg("host.refine")
    cfg, rooms, bank, room_model = _round_trip_room()
    rm, S = rooms[0], OC.ROUND_TRIP_S
    with torch.no_grad():
        render = R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), S).render(rm["boxes"], rm["angles"].float())[0]
    src_depth, src_labels = OB.observe(render)
    k_src, pose, K, orig = OC.round_trip_inputs(rm["boxes"][-1], S)
    rp = RP.ObservedReprojector(S, S, S, batch=1)
    depth, labels, hits = rp(src_depth, src_labels, k_src.cuda(), pose.cuda(), K.cuda(), orig)
    _sync("round trip of a device render")
    ok = OC.settled(src_depth.cpu(), src_labels.cpu()).cuda()
    hit = depth > 0
    err = float((depth - src_depth)[ok & hit].abs().max())
    print("round trip: %d settled pixels of %d, %d hits, settled without a hit %d, with another label %d, largest depth error %.3e (allowed %.3e)" % (
        int(ok.sum()), S * S, int(hits[0]), int((ok & ~hit).sum()), int((ok & (labels != src_labels)).sum()), err, 4 * ROUND_TRIP_F32_ERR))
    assert 2 * int(ok.sum()) >= S * S and len(set(src_labels[ok].tolist())) >= 4
    assert not bool((ok & ~hit).any()) and torch.equal(labels[ok], src_labels[ok]) and err <= 4.0 * ROUND_TRIP_F32_ERR
    assert int(hits[0]) == int(hit.sum())
    model, _ = room_model(cfg)
    rb = R.RefineBatch(model, rooms, observed=(depth, labels), bank=bank, learning_rate=1e-3, image_size=S, iters=1)
    try:
        losses = rb.run().cpu().numpy().copy()
        _sync("one iteration towards the reprojected pair")
        status = rb.target_status.tolist()
    finally:
        rb.close()
    assert np.isfinite(losses).all() and losses.shape[0] == 1
    assert status[0] & OB.STATUS_NO_WALL == 0, "the wall bit of target_status is clear"


def test_same_bytes_from_call_to_call_and_under_a_graph_replay():
    """T6"""
    L = _lib()
    c = OC.case("tile_edge_18x34_s32")
    args = _inputs(c)
    firsts = []
    try:
        for det in (0, 1):
            L.lib().sln_set_deterministic(det)
            rp, _ = _run(c)
            first = [t.clone() for t in (rp.depth, rp.labels, rp.hits, rp.faces_xyz)]
            for t in (rp.depth, rp.labels, rp.hits):
                t.fill_(3)
            rp(*args)
            _sync("second call")
            assert all(torch.equal(a, b) for a, b in zip(first, (rp.depth, rp.labels, rp.hits, rp.faces_xyz))) and torch.equal(_bits(first[0]), _bits(rp.depth))
            firsts.append(first)
    finally:
        L.lib().sln_set_deterministic(0)
    assert all(torch.equal(a, b) for a, b in zip(*firsts)), "either deterministic setting"
    first = firsts[0]
    args = tuple(a.clone() if torch.is_tensor(a) else a for a in args)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rp(*args)
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rp(*args)
    for _ in range(2):
        for t in (rp.depth, rp.labels, rp.hits, rp.faces_xyz):
            t.fill_(5)
        graph.replay()
        _sync("replay of the reprojection")
        assert all(torch.equal(a, b) for a, b in zip(first, (rp.depth, rp.labels, rp.hits, rp.faces_xyz))) and torch.equal(_bits(first[0]), _bits(rp.depth))
    # other contents through the same graph: frames 0 and 2 change places, with their cameras
    swap = [2, 1, 0]
    for a in args[:5]:
        a.copy_(a[swap].clone())
    graph.replay()
    _sync("replay with other contents")
    assert torch.equal(rp.hits, first[2][swap]) and torch.equal(_bits(rp.depth), _bits(first[0][swap])) and torch.equal(rp.labels, first[1][swap])


def test_refusals_leave_the_outputs_untouched():
    """T7"""
    L = _lib()
    RP = pkg("host.reproject")
    c = OC.case("slanted_3x5_s16")
    rp, out = _run(c)
    first = [t.clone() for t in out]
    junk = {"depth": 7.5, "labels": 9, "hits": -3, "faces_xyz": 2.5}
    for k, v in junk.items():
        getattr(rp, k).fill_(v)
    d, l, k, P, K, orig = _inputs(c)
    bad = [(d.cpu(), l, k, P, K, orig), (d.double(), l, k, P, K, orig), (d, l.to(torch.int32), k, P, K, orig), (d[:, :2].contiguous(), l, k, P, K, orig),
           (d, l, k[:, :3].contiguous(), P, K, orig), (d, l, k, P[:, :, :3].contiguous(), K, orig), (d, l, k, P, K.cpu(), orig),
           (d, l, k, P.transpose(1, 2).contiguous().transpose(1, 2), K, orig), (d, l, k, P, K, 0.0), (d, l, k, P, K, float("nan"))]
    for args in bad:
        with pytest.raises(ValueError):
            rp(*args)
    lib, ptr, st = L.lib(), L.ptr, L.current_stream_ptr()
    for kw in (dict(near=0.0), dict(gap=-1.0), dict(orig=0.0), dict(Hs=1), dict(B=0), dict(B=65536)):
        desc = L.SlnReproject()
        desc.depth_src, desc.k_src, desc.pose, desc.K_tgt = d.data_ptr(), k.data_ptr(), P.data_ptr(), K.data_ptr()
        desc.B, desc.Hs, desc.Ws = kw.get("B", 1), kw.get("Hs", 3), 5
        desc.orig_size, desc.near, desc.gap = kw.get("orig", 512.0), kw.get("near", 0.1), kw.get("gap", 0.05)
        assert lib.sln_reproject_faces(desc, ptr(rp.faces_xyz), st) == -1, kw
    for kw in (dict(S=4097), dict(S=0), dict(Hs=1), dict(B=0)):
        assert lib.sln_reproject_compose(ptr(rp.face_index), ptr(rp.weight), ptr(rp.raster_depth), ptr(l), kw.get("B", 1), kw.get("Hs", 3), 5, kw.get("S", 16),
                                         ptr(rp.depth), ptr(rp.labels), ptr(rp.hits), st) == -1, kw
    assert lib.sln_reproject_compose(ptr(rp.face_index), ptr(rp.weight), ptr(rp.raster_depth), ptr(l), 1, 3, 5, 16, ptr(rp.depth), ptr(rp.labels),
                                     C.c_void_p(rp.hits.data_ptr() + 4), st) == -1
    _sync("refused calls")
    for k_, v in junk.items():
        assert bool((getattr(rp, k_) == v).all()), k_
    rp(d, l, k, P, K, orig)                                          # ... and the same call with nothing wrong goes through
    _sync("the sound call")
    assert int(first[2][0]) > 0 and all(torch.equal(a, b) for a, b in zip(first, (rp.depth, rp.labels, rp.hits)))
