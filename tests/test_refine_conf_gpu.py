"""The refinement loss under a per-pixel confidence of the target on the device (DESIGN §4 "Refinement loss under per-pixel
confidence"): sln_refine_loss_confidence, the confidence instantiations of csrc/refine_loss.hip's loss / finalize / report kernels,
``RefineLoss(confidence=)``, ``RefineBatch(confidence=)`` and the one-room loops against ``refine.refinement_loss_confidence`` /
``confidence_counts_torch`` - the definition in torch ops - and, where the definition makes them coincide, against the bits of the masked
and the unmasked routes.  Targets, iterates and helpers are tests/test_refine_mask_gpu.py's (built once, shared, never modified);
tolerances are its too."""
import ctypes as C

import numpy as np
import pytest
import torch

import refine_conf_cases as CC
import refine_mask_cases as MC
import test_refine_mask_gpu as MG
from conftest import pkg
from oracle import vae_ref
from parity import assert_close

pytestmark = pytest.mark.gpu

CASES = MG.CASES
_CACHE = {}
_same_bytes, _fwd_bwd, _target_and_iterate, _dirty = MG._same_bytes, MG._fwd_bwd, MG._target_and_iterate, MG._dirty


def _conf(names, S):
    """uint8 [len(names), S, S] on the device"""
    return torch.from_numpy(np.stack([CC.pattern(n, S) for n in names])).cuda()


def _pair(name, batch):
    """the pattern for room 0 and, in a batch of two, the next pattern of the list for room 1"""
    k = CC.PATTERNS.index(name)
    return [name] + ([CC.PATTERNS[(k + 1) % len(CC.PATTERNS)]] if batch == 2 else [])


def _graded_pair(name, batch):
    k = CC.GRADED.index(name)
    return [name] + ([CC.GRADED[(k + 1) % len(CC.GRADED)]] if batch == 2 else [])


def _binary(batch, S):
    """(valid uint8 {0, 1}, the same as a confidence {0, 255}): rectangle for room 0, random holes for room 1"""
    valid = MG._valid(["rectangle", "random"][:batch], S)
    return valid, valid * 255


def _report(rl, img, target):
    """sln_refine_report behind a forward (it reads the forward's partial sums) -> [B, 3] on the host"""
    _lib = pkg("_lib")
    L = _lib.lib()
    B = img.shape[0]
    scratch = torch.zeros(int(L.sln_refine_report_scratch_doubles(B)), dtype=torch.float64, device="cuda")
    out = torch.full((B, 3), -9.0, device="cuda")
    tdepth = target[:, 41:].contiguous()
    _lib.check(L.sln_refine_report(rl.desc, _lib.ptr(img), _lib.ptr(tdepth), _lib.ptr(rl.ws), _lib.ptr(scratch), None, _lib.ptr(out),
                                   _lib.current_stream_ptr()), "sln_refine_report")
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------------------------------------
# 1: the set-up call against the host restatement, for equality
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size,batch", CASES)
def test_confidence_kernel_equals_the_host_restatement(image_size, batch):
    R, _lib = pkg("host.refine"), pkg("_lib")
    L = _lib.lib()
    sizes = CC.GEOMETRIES[image_size]
    ns, P = len(sizes), sizes[-1]
    target = _target_and_iterate(image_size, batch)[0].clone()
    q = image_size // 8
    target[:, 1:41, q:3 * q, 4 * q:7 * q] = 0.0                         # a window without a class: labels that are -100 before any confidence
    try:
        for per_room in (False, True):
            rl = R.RefineLoss(target, sizes, per_room)
            base = rl.labels.clone()
            assert int((base >= 0).sum()) > 0 and int((base < 0).sum()) > 0
            for name in CC.PATTERNS:
                conf = _conf(_pair(name, batch), image_size)
                want = R.confidence_counts_torch(conf.cpu(), base.cpu(), per_room, sizes)
                for det in (0, 1):
                    L.sln_set_deterministic(det)
                    for again in range(2):
                        # fresh labels, every output pre-filled with something else: nothing survives from the call before
                        lab = base.clone()
                        cp = torch.full((batch, ns, P, P), 9, dtype=torch.uint8, device="cuda")
                        inv = torch.full_like(rl.inv_count, -3.0)
                        cnt = torch.full((2, batch), -5, dtype=torch.int32, device="cuda")
                        csum = torch.full((2, batch), -11, dtype=torch.int64, device="cuda")
                        stat = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
                        _lib.check(L.sln_refine_loss_confidence(rl.desc, _lib.ptr(conf), _lib.ptr(lab), _lib.ptr(cp), _lib.ptr(inv), _lib.ptr(cnt),
                                                                _lib.ptr(csum), _lib.ptr(stat), _lib.ptr(rl.ws), _lib.current_stream_ptr()),
                                   "sln_refine_loss_confidence")
                        torch.cuda.synchronize()
                        where = "%s, per_room = %s, deterministic = %d, call %d" % (name, per_room, det, again)
                        assert torch.equal(cp.cpu(), want["conf_pooled"]), where
                        assert torch.equal(lab.cpu(), want["labels"]), where
                        assert torch.equal(cnt.cpu(), want["depth_count"]), where
                        assert torch.equal(csum.cpu(), want["conf_sum"]), where
                        assert stat.cpu().tolist() == want["mask_status"].tolist(), where
                        assert np.array_equal(inv.cpu().numpy().view(np.int32), want["inv_count"].numpy().view(np.int32)), where
    finally:
        L.sln_set_deterministic(0)


# ------------------------------------------------------------------------------------------------------------------------------
# 2: a {0, 255} confidence is the masked route, all 255 the unmasked one - bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_size,batch", CASES)
def test_binary_and_full_confidence_give_the_bits_of_the_existing_routes(image_size, batch):
    R = pkg("host.refine")
    sizes = CC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    valid, binary = _binary(batch, image_size)
    full = _conf(["full"] * batch, image_size)
    for per_room in (False, True):
        report = per_room or batch == 1
        masked, conf = R.RefineLoss(target, sizes, per_room, valid=valid), R.RefineLoss(target, sizes, per_room, confidence=binary)
        assert conf.conf_sum is not None and conf.desc.conf_sum and not masked.desc.conf_sum and masked.conf_sum is None
        assert torch.equal(conf.conf_pooled, masked.valid_pooled * 255) and torch.equal(conf.labels, masked.labels)
        assert _same_bytes(conf.inv_count, masked.inv_count) and torch.equal(conf.mask_count, masked.mask_count)
        assert torch.equal(conf.conf_sum, masked.mask_count.to(torch.int64) * 255) and conf.mask_status.tolist() == masked.mask_status.tolist()
        for generic in (False, True):
            (o0, g0), (o1, g1) = _fwd_bwd(masked, img, generic=generic), _fwd_bwd(conf, img, generic=generic)
            assert _same_bytes(o0, o1) and _same_bytes(g0, g1), "binary, per_room = %s, generic = %s" % (per_room, generic)
            assert bool(torch.isfinite(o0).all()) and float(g0.abs().max()) > 0
        if report:
            _fwd_bwd(masked, img); r0 = _report(masked, img, target)
            _fwd_bwd(conf, img); r1 = _report(conf, img, target)
            assert _same_bytes(r0[:, 1:], r1[:, 1:]) and bool(torch.isfinite(r0[:, 1:]).all()), (r0, r1)
        plain, conf = R.RefineLoss(target, sizes, per_room), R.RefineLoss(target, sizes, per_room, confidence=full)
        assert bool((conf.conf_pooled == 255).all()) and conf.mask_status.tolist() == [0] * batch
        assert torch.equal(plain.labels, conf.labels) and _same_bytes(plain.inv_count, conf.inv_count)
        for generic in (False, True):
            (o0, g0), (o1, g1) = _fwd_bwd(plain, img, generic=generic), _fwd_bwd(conf, img, generic=generic)
            assert _same_bytes(o0, o1) and _same_bytes(g0, g1), "full, per_room = %s, generic = %s" % (per_room, generic)
        if report:
            _fwd_bwd(plain, img); r0 = _report(plain, img, target)
            _fwd_bwd(conf, img); r1 = _report(conf, img, target)
            assert _same_bytes(r0[:, 1:], r1[:, 1:]), (r0, r1)


def test_binary_and_full_confidence_with_plane_flags_null_mask_and_pooled_ones():
    """live_planes / null_mask / pooled_ones supplied, as the rooms-in-flight loop hands them over (the image of
    test_all_ones_mask_with_plane_flags_null_mask_and_pooled_ones: dead semantic planes, a constant-1 depth-hot plane, null pixels)"""
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
    valid, binary = _binary(2, 96)
    full = _conf(["full"] * 2, 96)
    for per_room in (False, True):
        res = []
        for kw in (dict(valid=valid), dict(confidence=binary), dict(), dict(confidence=full)):
            rl = R.RefineLoss(target, per_room=per_room, **kw)
            keep = rl.pooled_ones()
            rl.desc.live_planes, rl.desc.null_mask, rl.desc.pooled_ones = live.data_ptr(), null.data_ptr(), keep.data_ptr()
            out, g = _fwd_bwd(rl, img)
            res.append((out, g, _report(rl, img, target) if per_room else None))
        for a, b, what in ((res[0], res[1], "binary"), (res[2], res[3], "full")):
            assert _same_bytes(a[0], b[0]) and _same_bytes(a[1], b[1]), (what, per_room)
            assert bool((a[1] == 7.0).any()) and bool(torch.isfinite(a[0]).all())
            if per_room:
                assert _same_bytes(a[2][:, 1:], b[2][:, 1:]), (what, a[2], b[2])
        assert not _same_bytes(res[0][0], res[2][0])


# ------------------------------------------------------------------------------------------------------------------------------
# 3: graded patterns against refinement_loss_confidence in fp64
# ------------------------------------------------------------------------------------------------------------------------------
def _reference(R, rl, target, img, conf, sizes):
    """refinement_loss_confidence on the CPU in fp64 and fp32 with the product's own labels: {dtype: ([loss, depth, sem], gradient)}"""
    labels = [rl.labels[:, k:k + 1].cpu().long() for k in range(rl.labels.shape[1])]
    ref = {}
    for dt in (torch.float64, torch.float32):
        xi = img.cpu().to(dt).requires_grad_(True)
        loss, dl, sl = R.refinement_loss_confidence(xi, target.cpu().to(dt), labels, torch.zeros((), dtype=dt), conf.cpu(), sizes)
        loss.backward()
        ref[dt] = ([float(loss.detach()), float(dl.detach()), float(sl.detach())], xi.grad.numpy())
    return ref


@pytest.mark.parametrize("name", CC.GRADED)
@pytest.mark.parametrize("image_size,batch", CASES)
def test_graded_confidence_matches_the_torch_restatement(image_size, batch, name):
    R = pkg("host.refine")
    sizes = CC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    conf = _conf(_graded_pair(name, batch), image_size)
    rl = R.RefineLoss(target, sizes, confidence=conf)
    x = img.clone().requires_grad_(True)
    out = rl(x)
    (out[0] * 1.5).backward()
    got = [float(t) for t in out.detach().cpu()]
    g = x.grad.cpu().numpy() / 1.5
    ref = _reference(R, rl, target, img, conf, sizes)
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
    # the grading is felt: the masked loss on the same support is another number, in both parts
    masked = R.RefineLoss(target, sizes, valid=(conf != 0).to(torch.uint8))(img).tolist()
    print("masked on the same support: %s" % (masked,))
    assert masked[1] != got[1] and masked[2] != got[2]
    if batch == 2:
        # per_room: every room is its own objective, normalised by its own sums - room b against the restatement on room b alone
        rlp = R.RefineLoss(target, sizes, per_room=True, confidence=conf)
        outp = rlp(img).cpu()
        for b in range(2):
            one = R.RefineLoss(target[b:b + 1], sizes, confidence=conf[b:b + 1])
            want = _reference(R, one, target[b:b + 1], img[b:b + 1], conf[b:b + 1], sizes)[torch.float64][0]
            for a, w in zip(outp[b].tolist(), want):
                assert abs(a - w) <= 1e-4 * abs(w) + 1e-7, (b, a, w)


# ------------------------------------------------------------------------------------------------------------------------------
# 4 / 5: what the target holds under confidence 0 does not matter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocks", "fused"])
@pytest.mark.parametrize("image_size,batch", CASES)
def test_content_under_zero_confidence_never_enters(image_size, batch, name):
    R = pkg("host.refine")
    sizes = CC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    conf = _conf(_graded_pair(name, batch), image_size)
    dirty = _dirty(target, conf)
    hole = (conf == 0)[:, None].expand_as(target)
    assert bool(hole[0].any()) and not bool(torch.isfinite(dirty[hole]).all()) and _same_bytes(dirty[~hole], target[~hole])
    for per_room in (False, True):
        clean_rl, dirty_rl = R.RefineLoss(target, sizes, per_room, confidence=conf), R.RefineLoss(dirty, sizes, per_room, confidence=conf)
        assert torch.equal(clean_rl.labels, dirty_rl.labels) and _same_bytes(clean_rl.inv_count, dirty_rl.inv_count)
        assert torch.equal(clean_rl.mask_count, dirty_rl.mask_count) and torch.equal(clean_rl.conf_sum, dirty_rl.conf_sum)
        (o0, g0), (o1, g1) = _fwd_bwd(clean_rl, img), _fwd_bwd(dirty_rl, img)
        assert bool(torch.isfinite(o1).all()) and bool(torch.isfinite(g1).all())
        assert _same_bytes(o0, o1) and _same_bytes(g0, g1), "per_room = %s" % per_room
        assert float(g1[:, 1:][hole[:, 1:]].abs().max()) == 0.0        # exactly 0 at every image pixel without confidence, planes 1..69
        assert float(g1.abs().max()) > 0
        if per_room or batch == 1:
            r0, r1 = _report(clean_rl, img, target), _report(dirty_rl, img, dirty)
            assert _same_bytes(r0[:, 1:], r1[:, 1:]) and bool(torch.isfinite(r1[:, 1:]).all())
        # the CSR-walk backward kernel: the same property, the same gradient
        o3, g3 = _fwd_bwd(dirty_rl, img, generic=True)
        assert _same_bytes(o3, o1) and float(g3[:, 1:][hole[:, 1:]].abs().max()) == 0.0 and bool(torch.isfinite(g3).all())
        assert_close(g3.cpu().numpy(), g1.cpu().numpy(), "generic vs separable backward", rtol=1e-5, atol=1e-6 * float(g1.abs().max()))


@pytest.mark.parametrize("image_size,batch", CASES)
def test_all_zeros_confidence(image_size, batch):
    R = pkg("host.refine")
    sizes = CC.GEOMETRIES[image_size]
    target, img = _target_and_iterate(image_size, batch)
    zeros = _conf(["zeros"] * batch, image_size)
    for per_room in (False, True):
        rl = R.RefineLoss(_dirty(target, zeros), sizes, per_room, confidence=zeros)
        assert rl.mask_status.tolist() == [3] * batch and not bool(rl.conf_pooled.any())
        assert not bool(rl.mask_count.any()) and not bool(rl.conf_sum.any())
        for generic in (False, True):
            out, g = _fwd_bwd(rl, img, generic=generic)
            assert float(out.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
        if per_room or batch == 1:
            rep = _report(rl, img, target)
            assert float(rep[:, 1:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# 6: descriptors that carry conf_sum without all of the mask's fields
# ------------------------------------------------------------------------------------------------------------------------------
def test_partial_confidence_descriptors_are_refused():
    R, _lib = pkg("host.refine"), pkg("_lib")
    L = _lib.lib()
    target, img = _target_and_iterate(96, 1)
    rl = R.RefineLoss(target, confidence=_conf(["blocks"], 96))
    fields = ("valid_pooled", "valid_image", "depth_count")
    out, gs, g = torch.empty(3, device="cuda"), torch.ones(1, device="cuda"), torch.zeros_like(img)
    pooled = torch.empty(1, 4, 69, 96, 96, device="cuda")
    scratch = torch.zeros(int(L.sln_refine_report_scratch_doubles(1)), dtype=torch.float64, device="cuda")
    rep = torch.empty(3, device="cuda")
    P, st = _lib.ptr, _lib.current_stream_ptr()
    tdepth = target[:, 41:].contiguous()
    for keep in range(0, 7):                                            # conf_sum with every proper subset of the three, the empty one included
        d = type(rl.desc).from_buffer_copy(rl.desc)
        for k, f in enumerate(fields):
            if not keep >> k & 1:
                setattr(d, f, None)
        assert d.conf_sum
        assert L.sln_refine_loss_init(C.byref(d), P(rl.ws), st) == -1, keep
        assert L.sln_refine_loss_live_ok(C.byref(d)) == 0, keep
        assert L.sln_refine_pool(C.byref(d), P(img), 0, P(rl.ws), P(pooled), st) == -1, keep
        assert L.sln_refine_loss_forward(C.byref(d), P(img), P(rl.target_depth), P(rl.labels), P(rl.inv_count), P(rl.ws), P(out), st) == -1, keep
        assert L.sln_refine_loss_backward(C.byref(d), P(rl.ws), P(gs), P(g), st) == -1, keep
        assert L.sln_refine_report(C.byref(d), P(img), P(tdepth), P(rl.ws), P(scratch), None, P(rep), st) == -1, keep
        assert L.sln_refine_loss_mask(C.byref(d), P(rl.conf), P(rl.labels), P(rl.conf_pooled), P(rl.inv_count), P(rl.mask_count), P(rl.mask_status),
                                      P(rl.ws), st) == -1, keep
        assert L.sln_refine_loss_confidence(C.byref(d), P(rl.conf), P(rl.labels), P(rl.conf_pooled), P(rl.inv_count), P(rl.mask_count), P(rl.conf_sum),
                                            P(rl.mask_status), P(rl.ws), st) == -1, keep
    d = type(rl.desc).from_buffer_copy(rl.desc)                          # the whole set goes through, and so does the mask alone
    assert L.sln_refine_loss_init(C.byref(d), P(rl.ws), st) == 0
    d.conf_sum = None
    assert L.sln_refine_loss_init(C.byref(d), P(rl.ws), st) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# 7: the loops
# ------------------------------------------------------------------------------------------------------------------------------
S, ITERS = 64, 4


def _setup():
    """model, two random rooms, and per room its own device render observed, cut into two overlapping halves (frame 0 keeps the columns
    <= 44, frame 1 the columns >= 20) and fused back by an ObservedFuser: the band both frames see has agree = 2, the rest 1, pixels
    without a winner 0 - ``ObservedFuser.confidence()`` of that is the loops' confidence"""
    if "rooms" not in _CACHE:
        import observed_reproject_cases as OC
        R, OB, RP = pkg("host.refine"), pkg("host.observe"), pkg("host.reproject")
        cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch", use_attr=False)
        model, sd = MG._room_model(cfg)
        rooms = MG._random_rooms(2, cfg, seed=11)
        bank = R.MeshBank(MG.FURN, "cuda", seed=3)
        with torch.no_grad():
            render = torch.cat([R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), S).render(rm["boxes"], rm["angles"].float())[0]
                                for rm in rooms], 0)
        src_depth, src_labels = OB.observe(render)                       # [2, S, S]
        per_room = [OC.round_trip_inputs(rm["boxes"][-1], S, B=2) for rm in rooms]
        assert per_room[0][3] == per_room[1][3]
        k_src, pose, K = (torch.stack([p[j] for p in per_room]).cuda() for j in range(3))
        depth_v, labels_v = src_depth[:, None].repeat(1, 2, 1, 1), src_labels[:, None].repeat(1, 2, 1, 1)
        depth_v[:, 0, :, 45:] = 0.0; labels_v[:, 0, :, 45:] = 0
        depth_v[:, 1, :, :20] = 0.0; labels_v[:, 1, :, :20] = 0
        fu = RP.ObservedFuser(S, S, S, rooms=2, views=2)
        depth, labels, _ = fu(depth_v.contiguous(), labels_v.contiguous(), k_src, pose, K[:, 0].contiguous(), per_room[0][3])
        conf = fu.confidence()
        assert conf.data_ptr() == fu.confidence().data_ptr()              # the static buffer
        torch.cuda.synchronize()
        want = (torch.clamp(fu.agree.to(torch.int32), max=2) * 255 + 1) // 2
        assert torch.equal(conf.to(torch.int32), want)
        levels = {int(v): int((conf == v).sum()) for v in conf.unique()}
        print("confidence of the fused pair: pixels per level %s" % levels)
        assert {128, 255} <= set(levels) <= {0, 128, 255} and min(levels[128], levels[255]) > S * S // 8, levels
        assert bool(((conf != 0) == (fu.source > 0)).all())
        _CACHE["rooms"] = dict(cfg=cfg, sd=sd, model=model, rooms=rooms, bank=bank, observed=(depth.clone(), labels.clone()), conf=conf.clone(),
                               kw=dict(bank=bank, learning_rate=1e-3, image_size=S, iters=ITERS))
    return _CACHE["rooms"]


def _run(R, s, rooms=None, capture=False, **kw):
    """a RefineBatch over ``rooms`` (default: both) run to the end under the deterministic switch -> dict of host copies"""
    L = pkg("_lib").lib()
    rb = None
    try:
        L.sln_set_deterministic(1)
        rb = R.RefineBatch(s["model"], s["rooms"] if rooms is None else rooms, **dict(s["kw"], **kw))
        losses = rb.run(capture=capture).clone()
        torch.cuda.synchronize()
        return dict(losses=losses, boxes=rb.boxes.clone(), idx=rb.idx.clone(), report=rb.report.clone() if rb._report_at is not None else None,
                    status=None if rb.mask_status is None else rb.mask_status.tolist(), row0=list(rb.row0), rows=list(rb.rows))
    finally:
        L.sln_set_deterministic(0)
        if rb is not None:
            rb.close()


def test_rooms_in_flight_under_a_binary_confidence_are_the_masked_rooms():
    R = pkg("host.refine")
    s = _setup()
    valid = (s["conf"] != 0).to(torch.uint8)
    a = _run(R, s, observed=s["observed"], mask=valid, report="all")
    b = _run(R, s, observed=s["observed"], confidence=valid * 255, report="all")
    assert a["status"] == b["status"] == [0, 0]
    assert _same_bytes(a["losses"], b["losses"]) and _same_bytes(a["boxes"], b["boxes"]) and _same_bytes(a["idx"], b["idx"])
    assert _same_bytes(a["report"][..., 1:], b["report"][..., 1:]) and bool(torch.isfinite(b["losses"]).all())
    # the fuser's graded confidence is another objective on the same support
    c = _run(R, s, observed=s["observed"], confidence=s["conf"], report="all")
    assert c["status"] == [0, 0] and not _same_bytes(c["losses"], a["losses"]) and bool(torch.isfinite(c["losses"]).all())
    assert bool(torch.isfinite(c["report"][..., 1:]).all())
    _CACHE["graded"] = c


def _graded(R, s):
    if "graded" not in _CACHE:
        _CACHE["graded"] = _run(R, s, observed=s["observed"], confidence=s["conf"], report="all")
    return _CACHE["graded"]


def test_one_room_of_two_and_a_graph_replay_give_the_eager_bits():
    R = pkg("host.refine")
    s = _setup()
    both = _graded(R, s)
    for r in range(2):
        one = _run(R, s, rooms=[s["rooms"][r]], observed=tuple(t[r:r + 1].contiguous() for t in s["observed"]),
                   confidence=s["conf"][r:r + 1].contiguous(), report="all")
        a, n = both["row0"][r], both["rows"][r]
        assert _same_bytes(one["losses"][:, 0], both["losses"][:, r]), r
        assert _same_bytes(one["boxes"], both["boxes"][a:a + n]) and _same_bytes(one["idx"], both["idx"][a:a + n]), r
        assert _same_bytes(one["report"][:, 0, 1:], both["report"][:, r, 1:]), r
    graph = _run(R, s, capture=True, observed=s["observed"], confidence=s["conf"], report="all")
    assert _same_bytes(graph["losses"], both["losses"]) and _same_bytes(graph["boxes"], both["boxes"]) and _same_bytes(graph["idx"], both["idx"])
    assert _same_bytes(graph["report"][..., 1:], both["report"][..., 1:])


def test_the_loops_against_the_autograd_yardstick():
    """RefineBatch(confidence=), finetune_vae_fast(confidence=) with and without the fused loss, finetune_vae(confidence=): one room's
    losses within what test_one_room_loop_with_an_observation_and_a_mask_equals_a_batch_of_one allows"""
    R = pkg("host.refine")
    s = _setup()
    rm = s["rooms"][1]
    obs, conf = tuple(t[1].contiguous() for t in s["observed"]), s["conf"][1].contiguous()          # [S, S]
    want = _graded(R, s)["losses"][:, 1].cpu().numpy()
    args = (rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"])
    kw = dict(iters=ITERS, bank=s["bank"], learning_rate=1e-3, image_size=S, observed=obs, confidence=conf)
    m1, _ = MG._room_model(s["cfg"], s["sd"])
    fast, _ = R.finetune_vae_fast(m1, *args, **kw)
    assert_close(fast.cpu().numpy(), want, "finetune_vae_fast(confidence=) vs RefineBatch", rtol=1e-5)
    m2, _ = MG._room_model(s["cfg"], s["sd"])
    torch_ops, _ = R.finetune_vae_fast(m2, *args, fused_loss=False, **kw)
    assert_close(torch_ops.cpu().numpy(), want, "finetune_vae_fast(fused_loss=False, confidence=) vs RefineBatch", rtol=2e-3)
    m3, _ = MG._room_model(s["cfg"], s["sd"])
    slow, _ = R.finetune_vae(m3, *args, **kw)
    print("RefineBatch %s, one-room loop %s, torch-op loss %s, reference-shaped loop %s" % (want.tolist(), fast.cpu().tolist(), torch_ops.cpu().tolist(), slow))
    assert_close(np.asarray(slow), want, "finetune_vae(confidence=) vs RefineBatch", rtol=2e-3)
    m4, _ = MG._room_model(s["cfg"], s["sd"])
    masked, _ = R.finetune_vae_fast(m4, *args, **dict(kw, confidence=None, mask=(conf != 0), iters=1))
    assert float(masked[0]) != float(fast[0])


def test_confidence_with_views():
    """V = 2: the [R, V, S, S] form.  Both views are the refinement view itself, so that image (r, v) is room r's image: with the
    room's confidence in both, the mean over the views is the one-view loss up to the float32 scale 1 / V of the gradients"""
    R, RP = pkg("host.refine"), pkg("host.reproject")
    s = _setup()
    cams = [RP.refine_view(rm["boxes"][-1], S)[:3] for rm in s["rooms"]]
    views = tuple(torch.stack([torch.stack([torch.as_tensor(c[j]).float().reshape(sh)] * 2) for c in cams]) for j, sh in enumerate(((3, 3), (3, 3), (3,))))
    obs = tuple(t[:, None].repeat(1, 2, 1, 1).contiguous() for t in s["observed"])
    conf = s["conf"][:, None].repeat(1, 2, 1, 1).contiguous()
    valid = (conf != 0).to(torch.uint8)
    a = _run(R, s, observed=obs, mask=valid, views=views)
    b = _run(R, s, observed=obs, confidence=valid * 255, views=views)
    assert a["status"] == b["status"] == [[0, 0], [0, 0]]
    assert _same_bytes(a["losses"], b["losses"]) and _same_bytes(a["boxes"], b["boxes"]) and _same_bytes(a["idx"], b["idx"])
    c = _run(R, s, observed=obs, confidence=conf, views=views)
    assert c["status"] == [[0, 0], [0, 0]] and bool(torch.isfinite(c["losses"]).all()) and not _same_bytes(c["losses"], a["losses"])
    assert_close(c["losses"].cpu().numpy(), _graded(R, s)["losses"].cpu().numpy(), "two copies of the view vs the one view", rtol=2e-3)
    with pytest.raises(ValueError):
        R.RefineBatch(s["model"], s["rooms"], observed=obs, confidence=s["conf"], views=views, **s["kw"])


class _Ordered:
    """the loaded library behind a proxy that lists every entry point looked up, in order (tests/test_refine_sequence_gpu.py's)"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


def _recorded(R, s, **kw):
    """_run with every library entry point the set-up and the loop look up listed -> (result, names)"""
    Lm = pkg("_lib")
    real = Lm.lib()
    Lm._lib = proxy = _Ordered(real)
    try:
        out = _run(R, s, **kw)
    finally:
        Lm._lib = real
    return out, proxy.calls


def test_no_confidence_is_the_default_run():
    """confidence=None: the bits and the sequence of library calls of a run that does not name the keyword"""
    R = pkg("host.refine")
    s = _setup()
    (a, calls_a), (b, calls_b) = _recorded(R, s), _recorded(R, s, confidence=None)
    assert calls_a == calls_b and len(calls_a) > ITERS
    assert "sln_refine_loss_confidence" not in calls_a and "sln_refine_loss_mask" not in calls_a
    assert a["status"] is None and b["status"] is None
    assert _same_bytes(a["losses"], b["losses"]) and _same_bytes(a["boxes"], b["boxes"]) and _same_bytes(a["idx"], b["idx"])
    # with a confidence: the one set-up call more, and the iterations' own calls unchanged
    c, calls_c = _recorded(R, s, confidence=s["conf"])
    assert calls_c.count("sln_refine_loss_confidence") == 1 and "sln_refine_loss_mask" not in calls_c
    rest = [n for n in calls_c if n != "sln_refine_loss_confidence"]
    assert rest == calls_a
    assert not _same_bytes(c["losses"], a["losses"])
