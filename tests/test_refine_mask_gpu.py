"""The refinement loss under a validity mask on the device (DESIGN §4 "Refinement loss under a validity mask"): sln_refine_loss_mask, the
masked instantiations of csrc/refine_loss.hip's loss / finalize / report kernels, ``RefineLoss(valid=)``, ``RefineBatch(mask=)`` and
``finetune_vae_fast(observed=, mask=)`` against ``refine.refinement_loss_masked`` / ``mask_counts_torch`` - the definition in torch ops.
Targets and iterates are those of tests/test_refine_gpu.py's loss tests (two renders of one room), the rooms those of its rooms-in-flight
tests; tolerances are test_fused_refinement_loss_matches_the_torch_ops's."""
import ctypes as C

import numpy as np
import pytest
import torch

import refine_mask_cases as MC
from conftest import pkg
from oracle import vae_ref
from parity import assert_close

pytestmark = pytest.mark.gpu

NAMES = ["bed", "chair", "table", "sofa", "door", "desk", "__room__"]
FURN = ["bed", "chair", "table", "sofa", "desk", "cabinet", "lamp", "television", "bookshelf", "dresser", "night_stand", "shelves"]
CASES = [(96, 1), (96, 2), (40, 1)]             # (image size, batch); 40: three scales (8, 12, 16), P * P = 256
_CACHE = {}


def _inputs(dev):
    g = torch.Generator().manual_seed(0)
    lo = torch.rand(len(NAMES), 3, generator=g) * 0.45 + 0.05
    lo[:, 1] = 0.0; lo[:, 2] = lo[:, 2] * 0.6
    hi = lo + torch.rand(len(NAMES), 3, generator=g) * 0.2 + 0.12
    boxes = torch.cat([lo, hi], 1)
    boxes[-1] = torch.tensor([0, 0, 0, 4.0, 2.7, 5.0])
    angles = torch.randint(0, 24, (len(NAMES),), generator=g).float()
    return boxes.to(dev), angles.to(dev)


def _target_and_iterate(image_size, batch):
    """Two renders of the same room, the second with its objects moved and turned (as tests/test_refine_gpu.py makes them); built once
    per geometry and never modified"""
    key = ("ti", image_size, batch)
    if key not in _CACHE:
        R = pkg("host.refine"); DR = pkg("host.diff_render")
        boxes, angles = _inputs("cuda")
        bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], "cuda", seed=3)
        room = boxes[-1].clone()
        v0, f0, ranges, _, _ = R.assemble_scene(boxes, angles, NAMES, bank, room)
        with torch.no_grad():
            target = DR.scene_render(v0, f0, ranges, room, image_size=image_size)
            b2 = boxes + 0.03; b2[-1] = boxes[-1]
            v, f, ranges, _, _ = R.assemble_scene(b2, angles + 0.7, NAMES, bank, room)
            img = DR.scene_render(v, f, ranges, room, image_size=image_size)
            if batch == 2:
                target, img = torch.cat([target, img]), torch.cat([img, target])
        _CACHE[key] = (target, img)
    return _CACHE[key]


def _valid(names, S):
    """uint8 [len(names), S, S] on the device"""
    return torch.from_numpy(np.stack([MC.pattern(n, S) for n in names])).cuda()


def _pair(name, batch):
    """the pattern for room 0 and, in a batch of two, the next pattern of the list for room 1"""
    k = MC.PATTERNS.index(name)
    return [name] + ([MC.PATTERNS[(k + 1) % len(MC.PATTERNS)]] if batch == 2 else [])


def _dirty(target, valid):
    """NaN, +inf and 1e30 (in turns) in all 70 planes wherever valid == 0"""
    t = target.clone()
    hole = (valid == 0)[:, None].expand_as(t)
    turn = (torch.arange(t.numel(), device=t.device).reshape(t.shape) % 3)
    for k, val in enumerate((float("nan"), float("inf"), 1e30)):
        t[hole & (turn == k)] = val
    return t


class _Generic:
    """a RefineLoss seen through a copy of its descriptor that does not know the longest CSR row (max_col_entries = 0)"""

    def __init__(self, rl):
        self.__dict__.update(rl.__dict__)
        self.desc = type(rl.desc).from_buffer_copy(rl.desc)
        self.desc.max_col_entries = 0


def _fwd_bwd(rl, img, gscale=1.5, generic=False):
    """the two C calls on a gradient buffer that holds a sentinel (planes nobody reads the gradient of keep it) -> (out, grad)"""
    _lib = pkg("_lib")
    L = _lib.lib()
    out = torch.empty((img.shape[0], 3) if rl.per_room else (3,), device="cuda")
    g = torch.full(img.shape, 7.0, device="cuda")
    gs = torch.full((1,), gscale, device="cuda")
    st = _lib.current_stream_ptr()
    if generic:                                                        # 'unknown': the CSR-walk backward kernel instead of the separable one
        rl = _Generic(rl)
    _lib.check(L.sln_refine_loss_forward(rl.desc, _lib.ptr(img), _lib.ptr(rl.target_depth), _lib.ptr(rl.labels), _lib.ptr(rl.inv_count), _lib.ptr(rl.ws),
                                         _lib.ptr(out), st), "sln_refine_loss_forward")
    _lib.check(L.sln_refine_loss_backward(rl.desc, _lib.ptr(rl.ws), _lib.ptr(gs), _lib.ptr(g), st), "sln_refine_loss_backward")
    torch.cuda.synchronize()
    return out, g


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------
# T1: an all-ones mask is the unmasked loss, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size,batch", CASES)
def test_all_ones_mask_gives_the_bits_of_the_unmasked_loss(image_size, batch):
    R = pkg("host.refine")
    sizes = MC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    ones = torch.ones(batch, image_size, image_size, dtype=torch.uint8, device="cuda")
    for per_room in (False, True):
        rl0, rl1 = R.RefineLoss(target, sizes, per_room), R.RefineLoss(target, sizes, per_room, valid=ones)
        assert rl0.valid_pooled is None and rl0.mask_status is None and not rl0.desc.valid_pooled
        assert bool(rl1.valid_pooled.all()) and rl1.mask_status.tolist() == [0] * batch
        assert torch.equal(rl0.labels, rl1.labels) and _same_bytes(rl0.inv_count, rl1.inv_count)
        (o0, g0), (o1, g1) = _fwd_bwd(rl0, img), _fwd_bwd(rl1, img)
        assert _same_bytes(o0, o1) and _same_bytes(g0, g1), "per_room = %s" % per_room
        assert bool(torch.isfinite(o0).all()) and float(g0.abs().max()) > 0


def test_all_ones_mask_with_plane_flags_null_mask_and_pooled_ones():
    """live_planes / null_mask / pooled_ones supplied, as the rooms-in-flight loop hands them over (the image of
    test_fused_refinement_loss_with_plane_flags_and_neither_optional_table: dead semantic planes, a constant-1 depth-hot plane, null pixels)"""
    R = pkg("host.refine")
    target, img = _target_and_iterate(96, 2)
    img = img.clone()
    flat = [c for c in range(41, 69) if float(img[0, c].min()) == float(img[0, c].max())]
    assert flat, "no constant depth-hot plane in sample 0"
    img[:, 41:, 10:40, 20:70] = 0.0
    img[0, flat[0]] = 1.0
    live = torch.full(img.shape[:2], 3, dtype=torch.uint8)
    host = img.cpu()
    for b in range(2):
        for c in range(1, 69):
            if not bool(host[b, c].any()):
                live[b, c] = 0
            elif c >= 41 and bool((host[b, c] == 1.0).all()):
                live[b, c] = 1
    assert (live[:, 1:41] == 0).any() and (live[0, 41:] == 1).any()
    live = live.cuda()
    null = (img[:, 41:].sum(1) < 0.5).to(torch.uint8).contiguous()
    assert bool(null[1].any())
    ones = torch.ones(2, 96, 96, dtype=torch.uint8, device="cuda")
    res = []
    for valid in (None, ones):
        rl = R.RefineLoss(target, per_room=True, valid=valid)
        keep = rl.pooled_ones()
        rl.desc.live_planes, rl.desc.null_mask, rl.desc.pooled_ones = live.data_ptr(), null.data_ptr(), keep.data_ptr()
        res.append(_fwd_bwd(rl, img))
    assert _same_bytes(res[0][0], res[1][0]) and _same_bytes(res[0][1], res[1][1])
    assert bool((res[0][1] == 7.0).any()) and bool(torch.isfinite(res[0][0]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# T2: the set-up call against the host restatement, for equality
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size,batch", CASES)
def test_mask_kernel_equals_the_host_restatement(image_size, batch):
    R, _lib = pkg("host.refine"), pkg("_lib")
    L = _lib.lib()
    sizes = MC.GEOMETRIES[image_size]
    ns, P = len(sizes), sizes[-1]
    target = _target_and_iterate(image_size, batch)[0].clone()
    q = image_size // 8
    target[:, 1:41, q:3 * q, 4 * q:7 * q] = 0.0                         # a window without a class: labels that are -100 before any mask
    try:
        for per_room in (False, True):
            rl = R.RefineLoss(target, sizes, per_room)
            base = rl.labels.clone()
            assert int((base >= 0).sum()) > 0 and int((base < 0).sum()) > 0
            for name in MC.PATTERNS:
                valid = _valid(_pair(name, batch), image_size)
                want = R.mask_counts_torch(valid.cpu(), base.cpu(), per_room, sizes)
                for det in (0, 1):
                    L.sln_set_deterministic(det)
                    for again in range(2):
                        # fresh labels, every output pre-filled with something else: nothing survives from the call before
                        lab = base.clone()
                        vp = torch.full((batch, ns, P, P), 9, dtype=torch.uint8, device="cuda")
                        inv = torch.full_like(rl.inv_count, -3.0)
                        cnt = torch.full((2, batch), -5, dtype=torch.int32, device="cuda")
                        stat = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
                        _lib.check(L.sln_refine_loss_mask(rl.desc, _lib.ptr(valid), _lib.ptr(lab), _lib.ptr(vp), _lib.ptr(inv), _lib.ptr(cnt),
                                                          _lib.ptr(stat), _lib.ptr(rl.ws), _lib.current_stream_ptr()), "sln_refine_loss_mask")
                        torch.cuda.synchronize()
                        where = "%s, per_room = %s, deterministic = %d, call %d" % (name, per_room, det, again)
                        assert torch.equal(vp.cpu(), want["valid_pooled"]), where
                        assert torch.equal(lab.cpu(), want["labels"]), where
                        assert torch.equal(cnt.cpu(), want["depth_count"]), where
                        assert stat.cpu().tolist() == want["mask_status"].tolist(), where
                        assert np.array_equal(inv.cpu().numpy().view(np.int32), want["inv_count"].numpy().view(np.int32)), where
    finally:
        L.sln_set_deterministic(0)


# ------------------------------------------------------------------------------------------------------------------------------
# T3: values against refinement_loss_masked in fp64
# ------------------------------------------------------------------------------------------------------------------------------
def _reference(R, rl, target, img, valid, sizes):
    """refinement_loss_masked on the CPU in fp64 and fp32 with the product's own (masked) labels: {dtype: ([loss, depth, sem], gradient)}"""
    labels = [rl.labels[:, k:k + 1].cpu().long() for k in range(rl.labels.shape[1])]
    ref = {}
    for dt in (torch.float64, torch.float32):
        xi = img.cpu().to(dt).requires_grad_(True)
        loss, dl, sl = R.refinement_loss_masked(xi, target.cpu().to(dt), labels, torch.zeros((), dtype=dt), valid.cpu(), sizes)
        loss.backward()
        ref[dt] = ([float(loss.detach()), float(dl.detach()), float(sl.detach())], xi.grad.numpy())
    return ref


@pytest.mark.parametrize("name", ["rectangle", "random"])
@pytest.mark.parametrize("image_size,batch", CASES)
def test_masked_loss_matches_the_torch_restatement(image_size, batch, name):
    R = pkg("host.refine")
    sizes = MC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    valid = _valid(_pair(name, batch), image_size)
    rl = R.RefineLoss(target, sizes, valid=valid)
    x = img.clone().requires_grad_(True)
    out = rl(x)
    (out[0] * 1.5).backward()
    got = [float(t) for t in out.detach().cpu()]
    g = x.grad.cpu().numpy() / 1.5
    ref = _reference(R, rl, target, img, valid, sizes)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    print("loss (total, depth, semantic): device %s, fp64 %s" % (got, r64[0]))
    for a, b, nm in zip(got, r64[0], ("total", "depth", "semantic")):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (nm, a, b)
    scale = np.abs(r64[1]).max()
    bad = np.abs(g - r64[1]) > 1e-4 * scale
    bad32 = np.abs(r32[1] - r64[1]) > 1e-4 * scale
    print("gradient: outliers %.3g (fp32 restatement %.3g), max error %.3g (fp32 restatement %.3g), scale %.3g" % (
        bad.mean(), bad32.mean(), np.abs(g - r64[1]).max(), np.abs(r32[1] - r64[1]).max(), scale))
    assert scale > 0 and (g[:, 0] == 0).all()
    assert bad.mean() <= max(4.0 * bad32.mean(), 1e-5), (bad.mean(), bad32.mean())
    assert np.abs(g - r64[1]).max() <= 1e-4 * scale + 4.0 * np.abs(r32[1] - r64[1]).max()
    # the mask is felt: the unmasked loss of the same pair is another number
    assert float(R.RefineLoss(target, sizes)(img)[1]) != got[1]
    if batch == 2:
        # per_room: every room is its own objective, normalised by its own counts - room b against the restatement on room b alone
        rlp = R.RefineLoss(target, sizes, per_room=True, valid=valid)
        outp = rlp(img).cpu()
        for b in range(2):
            one = R.RefineLoss(target[b:b + 1], sizes, valid=valid[b:b + 1])
            want = _reference(R, one, target[b:b + 1], img[b:b + 1], valid[b:b + 1], sizes)[torch.float64][0]
            for a, w in zip(outp[b].tolist(), want):
                assert abs(a - w) <= 1e-4 * abs(w) + 1e-7, (b, a, w)


# ------------------------------------------------------------------------------------------------------------------------------
# T4 / T5: what the target holds under the mask does not matter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rectangle", "random"])
@pytest.mark.parametrize("image_size,batch", CASES)
def test_content_under_the_mask_never_enters(image_size, batch, name):
    R = pkg("host.refine")
    sizes = MC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    valid = _valid(_pair(name, batch), image_size)
    dirty = _dirty(target, valid)
    hole = (valid == 0)[:, None].expand_as(target)
    assert not bool(torch.isfinite(dirty[hole]).all()) and _same_bytes(dirty[~hole], target[~hole])
    for per_room in (False, True):
        clean_rl, dirty_rl = R.RefineLoss(target, sizes, per_room, valid=valid), R.RefineLoss(dirty, sizes, per_room, valid=valid)
        assert torch.equal(clean_rl.labels, dirty_rl.labels) and _same_bytes(clean_rl.inv_count, dirty_rl.inv_count)
        assert torch.equal(clean_rl.mask_count, dirty_rl.mask_count)
        (o0, g0), (o1, g1) = _fwd_bwd(clean_rl, img), _fwd_bwd(dirty_rl, img)
        assert bool(torch.isfinite(o1).all()) and bool(torch.isfinite(g1).all())
        assert _same_bytes(o0, o1) and _same_bytes(g0, g1), "per_room = %s" % per_room
        assert float(g1[:, 1:][hole[:, 1:]].abs().max()) == 0.0        # exactly 0 at every invalid image pixel of planes 1..69
        assert float(g1.abs().max()) > 0
        # the CSR-walk backward kernel (the separable one takes both geometries): the same property, the same gradient
        o3, g3 = _fwd_bwd(dirty_rl, img, generic=True)
        assert _same_bytes(o3, o1) and float(g3[:, 1:][hole[:, 1:]].abs().max()) == 0.0 and bool(torch.isfinite(g3).all())
        assert_close(g3.cpu().numpy(), g1.cpu().numpy(), "generic vs separable backward", rtol=1e-5, atol=1e-6 * float(g1.abs().max()))
        # iterate == target (the clean one): the depth part vanishes exactly, and so do the depth planes' gradients
        o2, g2 = _fwd_bwd(dirty_rl, target)
        assert float(o2.reshape(-1, 3)[:, 1].abs().max()) == 0.0
        assert float(g2[:, 41:-1].abs().max()) == 0.0
        null = target[:, 41:].sum(1) < 0.5
        assert float(g2[:, -1][null].abs().max() if bool(null.any()) else 0.0) == 0.0 and bool(torch.isfinite(g2).all())


@pytest.mark.parametrize("image_size,batch", CASES)
def test_all_invalid_mask(image_size, batch):
    R = pkg("host.refine")
    sizes = MC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    zeros = torch.zeros(batch, image_size, image_size, dtype=torch.uint8, device="cuda")
    checker = _valid(["checkerboard"] * batch, image_size)               # pools to all-invalid although half of its pixels are valid
    for valid in (zeros, checker):
        for per_room in (False, True):
            rl = R.RefineLoss(_dirty(target, valid), sizes, per_room, valid=valid)
            out, g = _fwd_bwd(rl, img)
            assert rl.mask_status.tolist() == [3] * batch and not bool(rl.valid_pooled.any())
            assert rl.mask_count[0].tolist() == [0] * batch and rl.mask_count[1].tolist() == [int(v.sum()) for v in valid]
            assert float(out.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
            out, g = _fwd_bwd(rl, img, generic=True)
            assert float(out.abs().max()) == 0.0 and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# T6 / T7: RefineBatch(mask=), finetune_vae_fast(observed=, mask=)
# ------------------------------------------------------------------------------------------------------------------------------
S = 96


def _random_rooms(n_rooms, cfg, seed=0, dev="cuda"):
    """rooms of 4 .. 13 objects (+ the room row), as tests/test_refine_gpu.py draws them"""
    rng = np.random.default_rng(seed)
    rooms = []
    for r in range(n_rooms):
        k = int(rng.integers(4, 14))
        names = [FURN[int(i)] for i in rng.integers(0, len(FURN), k)] + ["__room__"]
        n = k + 1
        lo = rng.uniform(0.05, 0.5, (n, 3)); lo[:, 1] = 0.0; lo[:, 2] *= 0.6
        hi = lo + rng.uniform(0.12, 0.32, (n, 3))
        boxes = np.concatenate([lo, hi], 1).astype(np.float32)
        boxes[-1] = [0, 0, 0, 3.5 + rng.uniform(0, 1), 2.7, 4.5 + rng.uniform(0, 1)]
        objs = np.concatenate([rng.integers(1, cfg.num_objs, k), [0]])
        tri = [[i, int(rng.integers(1, cfg.num_preds)), int((i + 1 + rng.integers(0, k - 1)) % k)] for i in range(k)] + [[i, 0, k] for i in range(k)]
        rooms.append(dict(objs=torch.tensor(objs, device=dev), triples=torch.tensor(tri, device=dev), boxes=torch.from_numpy(boxes).to(dev),
                          angles=torch.tensor(rng.integers(0, 24, n), device=dev), attributes=torch.tensor(rng.integers(0, cfg.num_attrs, n), device=dev),
                          class_names=names))
    return rooms


def _room_model(cfg, sd=None, seed=1):
    M = pkg("host.Sg2ScVAE_model")
    if sd is None:
        sd = vae_ref.init_state(cfg, seed=seed, scale=0.3)
        last = "box_net.%d.bias" % (3 if cfg.mlp_normalization == "batch" else 2)
        sd[last] = torch.tensor([0.25, 0.0, 0.2, 0.55, 0.35, 0.5])
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    return model.cuda().eval(), sd


def _setup():
    """model, two random rooms, their own renders observed, and the same observation with a rectangular hole punched into room 1 only"""
    if "rooms" not in _CACHE:
        R, OB = pkg("host.refine"), pkg("host.observe")
        cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch", use_attr=False)
        model, sd = _room_model(cfg)
        rooms = _random_rooms(2, cfg, seed=11)
        bank = R.MeshBank(FURN, "cuda", seed=3)
        with torch.no_grad():
            render = torch.cat([R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), S).render(rm["boxes"], rm["angles"].float())[0]
                                for rm in rooms], 0)
        depth, labels = OB.observe(render)
        holed_d, holed_l = depth.clone(), labels.clone()
        holed_d[1, 30:55, 25:70] = 0.0
        holed_l[1, 30:55, 25:70] = 0
        torch.cuda.synchronize()
        _CACHE["rooms"] = dict(cfg=cfg, sd=sd, model=model, rooms=rooms, bank=bank, render=render, full=(depth, labels), holed=(holed_d, holed_l),
                               kw=dict(bank=bank, learning_rate=1e-3, image_size=S, iters=3))
    return _CACHE["rooms"]


def _image_as_the_loss_saw_it(rb, r):
    """room r's iterate with the planes the scene pass leaves unwritten put back: zeros (the buffer's), or the constant 1 of its flag"""
    img = rb.image[r:r + 1].clone()
    img[0, (rb.live[r] == 1).nonzero().flatten()] = 1.0
    return img


def test_rooms_in_flight_under_a_mask_of_readings():
    R, OB, L = pkg("host.refine"), pkg("host.observe"), pkg("_lib").lib()
    s = _setup()
    try:
        L.sln_set_deterministic(1)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            masked = R.RefineBatch(s["model"], s["rooms"], observed=s["holed"], mask="readings", report="all", **s["kw"])
            masked.run(1)
            torch.cuda.synchronize()
            first = dict(img=_image_as_the_loss_saw_it(masked, 1).cpu(), out=masked.loss_out[1].cpu().tolist(), report=masked.report[0, 1].cpu().tolist(),
                         size=float(masked.size_loss[1]), loss=float(masked.losses[0, 1]))
            masked.run()
            plain = R.RefineBatch(s["model"], s["rooms"], observed=s["full"], **s["kw"])
            plain.run()
            graph = R.RefineBatch(s["model"], s["rooms"], observed=s["holed"], mask="readings", report="all", **s["kw"])
            graph.run(capture=True)
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    try:
        assert plain.mask_status is None and masked.mask_status.tolist() == [0, 0]
        valid = masked.loss.valid
        holes = [int((v == 0).sum()) for v in valid]
        print("invalid pixels per room:", holes, " valid pooled pixels:", masked.loss.mask_count[0].tolist())
        assert holes[1] >= 25 * 45
        # room 0: no hole - the bytes of the run without a hole and without a mask
        a, n = masked.row0[0], masked.rows[0]
        assert holes[0] == 0, "room 0's own render leaves pixels without a reading: choose a room that fills the view"
        assert _same_bytes(masked.losses[:, 0], plain.losses[:, 0])
        assert _same_bytes(masked.boxes[a:a + n], plain.boxes[a:a + n]) and _same_bytes(masked.idx[a:a + n], plain.idx[a:a + n])
        assert not _same_bytes(masked.losses[:, 1], plain.losses[:, 1])
        # the graph replays to the eager bytes
        assert _same_bytes(graph.losses, masked.losses) and _same_bytes(graph.boxes, masked.boxes) and _same_bytes(graph.report, masked.report)
        # room 1, first iteration: the loss against the torch restatement on the same tensors
        target, _ = OB.ObservedTarget(masked.chan, masked.dch, S, batch=2)(*s["holed"])
        t1, v1 = target[1:2].cpu(), valid[1:2].cpu()
        assert bool(((t1[:, 0] >= 0) == (v1 != 0)).all())
        labels = [masked.loss.labels[1:2, k:k + 1].cpu().long() for k in range(4)]
        want = [float(x) for x in R.refinement_loss_masked(first["img"].double(), t1.double(), labels, torch.zeros((), dtype=torch.float64), v1)]
        print("room 1, iteration 0: device %s, fp64 %s" % (first["out"], want))
        for got, w in zip(first["out"], want):
            assert abs(got - w) <= 1e-4 * abs(w) + 1e-7, (got, w)
        assert abs(first["loss"] - (first["out"][0] + 2.0 * first["size"])) <= 1e-6 * abs(first["loss"])
        # the report's depth_l1: the mean over the valid pixels of the 29 planes, the iterate null-filled (:332)
        it = first["img"].double()[0, 41:].clone()
        it[-1][it.sum(0) < 0.5] = 1.0
        diff = (it - t1.double()[0, 41:]).abs()[:, v1[0] != 0]
        assert abs(first["report"][1] - float(diff.mean())) <= 1e-5 * float(diff.mean()), (first["report"], float(diff.mean()))
        assert np.isfinite(masked.report.cpu().numpy()).all()
    finally:
        for rb in (masked, plain, graph):
            rb.close()


def test_a_tensor_mask_on_rendered_targets_and_the_refusals():
    R = pkg("host.refine")
    s = _setup()
    mask = torch.ones(2, S, S, dtype=torch.bool, device="cuda")
    mask[0, 10:30, 40:90] = False
    rb = R.RefineBatch(s["model"], s["rooms"], mask=mask, report="ends", **s["kw"])
    rb0 = R.RefineBatch(s["model"], s["rooms"], **s["kw"])
    try:
        losses, plain = rb.run().cpu().numpy(), rb0.run().cpu().numpy()
        assert np.isfinite(losses).all() and np.isfinite(rb.report[0].cpu().numpy()[:, 1:]).all() and rb.mask_status.tolist() == [0, 0]
        assert (losses[:, 0] != plain[:, 0]).any()
        assert_close(losses[:, 1], plain[:, 1], "the unmasked room of a masked batch", rtol=1e-5)
    finally:
        rb.close(); rb0.close()
    with pytest.raises(ValueError):
        R.RefineBatch(s["model"], s["rooms"], mask="readings", **s["kw"])
    ok = mask.to(torch.uint8)
    for bad in (ok[:1].contiguous(), ok[:, :48].contiguous(), ok.float(), ok.to(torch.int32), ok.cpu(), "holes"):
        with pytest.raises(ValueError):
            R.RefineBatch(s["model"], s["rooms"], mask=bad, **s["kw"])
        with pytest.raises(ValueError):
            R.RefineLoss(s["render"], per_room=True, valid=bad)


def test_one_room_loop_with_an_observation_and_a_mask_equals_a_batch_of_one():
    R = pkg("host.refine")
    s = _setup()
    rm = s["rooms"][1]
    obs = (s["holed"][0][1].contiguous(), s["holed"][1][1].contiguous())          # [S, S]
    rb = R.RefineBatch(s["model"], [rm], observed=(obs[0][None], obs[1][None]), mask="readings", **s["kw"])
    try:
        want = rb.run().cpu().numpy()[:, 0].copy()
        assert rb.mask_status.tolist() == [0]
    finally:
        rb.close()
    m1, _ = _room_model(s["cfg"], s["sd"])
    losses, _ = R.finetune_vae_fast(m1, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=3,
                                    bank=s["bank"], learning_rate=1e-3, image_size=S, observed=obs, mask="readings")
    print("one-room loop %s, batch of one %s" % (losses.cpu().tolist(), want.tolist()))
    assert_close(losses.cpu().numpy(), want, "finetune_vae_fast(observed=, mask='readings') vs RefineBatch", rtol=1e-5)
    m2, _ = _room_model(s["cfg"], s["sd"])
    unmasked, _ = R.finetune_vae_fast(m2, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=1,
                                      bank=s["bank"], learning_rate=1e-3, image_size=S, observed=obs)
    assert float(unmasked[0]) != float(losses[0])
    # the torch-op routes of the same arguments: finetune_vae_fast without the fused loss and the reference-shaped loop, both through
    # refinement_loss_masked - within what test_fast_finetune_loop_matches_the_reference_shaped_loop_and_its_graph_replay allows
    m3, _ = _room_model(s["cfg"], s["sd"])
    torch_ops, _ = R.finetune_vae_fast(m3, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=3,
                                       bank=s["bank"], learning_rate=1e-3, image_size=S, observed=obs, mask="readings", fused_loss=False)
    assert_close(torch_ops.cpu().numpy(), losses.cpu().numpy(), "finetune_vae_fast(fused_loss=False) vs the fused loss", rtol=2e-3)
    m4, _ = _room_model(s["cfg"], s["sd"])
    slow, _ = R.finetune_vae(m4, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=3,
                             bank=s["bank"], learning_rate=1e-3, image_size=S, observed=obs, mask="readings")
    print("torch-op loss %s, reference-shaped loop %s" % (torch_ops.cpu().tolist(), slow))
    assert_close(np.asarray(slow), losses.cpu().numpy(), "finetune_vae(observed=, mask='readings') vs finetune_vae_fast", rtol=2e-3)


# ------------------------------------------------------------------------------------------------------------------------------
# T8: descriptors that set some but not all of the mask's fields
# ------------------------------------------------------------------------------------------------------------------------------
def test_partial_mask_descriptors_are_refused():
    R, _lib = pkg("host.refine"), pkg("_lib")
    L = _lib.lib()
    target, img = _target_and_iterate(96, 1)
    rl = R.RefineLoss(target, valid=_valid(["rectangle"], 96))
    fields = ("valid_pooled", "valid_image", "depth_count")
    out = torch.empty(3, device="cuda")
    for keep in range(1, 7):                                            # every proper, non-empty subset of the three
        d = type(rl.desc).from_buffer_copy(rl.desc)
        for k, f in enumerate(fields):
            if not keep >> k & 1:
                setattr(d, f, None)
        assert L.sln_refine_loss_init(C.byref(d), _lib.ptr(rl.ws), _lib.current_stream_ptr()) == -1, keep
        assert L.sln_refine_loss_forward(C.byref(d), _lib.ptr(img), _lib.ptr(rl.target_depth), _lib.ptr(rl.labels), _lib.ptr(rl.inv_count),
                                         _lib.ptr(rl.ws), _lib.ptr(out), _lib.current_stream_ptr()) == -1, keep
    for keep in (0, 7):
        d = type(rl.desc).from_buffer_copy(rl.desc)
        if keep == 0:
            d.valid_pooled = d.valid_image = d.depth_count = None
        assert L.sln_refine_loss_init(C.byref(d), _lib.ptr(rl.ws), _lib.current_stream_ptr()) == 0
    torch.cuda.synchronize()
