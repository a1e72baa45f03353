"""Several target views per room inside the refinement loops (``views=`` of RefineBatch, finetune_vae_fast_batch and finetune_vae; DESIGN §4
"Several target views per room"): the set-up of tests/test_refine_overlap_gpu.py - two synthetic rooms of tests/test_refine_gpu.py at
64 x 64, four iterations, deterministic mode.  View 0 is the refinement camera, view 1 looks from an upper corner of the room at its
centre.  Tolerances between loops are those tests/test_refine_gpu.py uses for the same pairs of loops."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

import test_refine_gpu as TR
from test_refine_overlap_gpu import CFG, IMAGE, ITERS, WEIGHT, _same_bits, _setup

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cameras():
    """(K [2, 2, 3, 3], Rm [2, 2, 3, 3], t [2, 2, 3]) on the host: per room the refinement camera and the corner view"""
    RP = pkg("host.reproject")
    _, _, rooms, _ = _setup()
    cams = []
    for rm in rooms:
        ext = rm["boxes"][-1, 3:].cpu().double().numpy()
        cams.append([RP.refine_view(rm["boxes"][-1], IMAGE)[:3], RP.look_at_view(ext * [0.9, 0.9, 0.9], ext / 2)[:3]])
    return tuple(torch.stack([torch.stack([cams[r][v][j] for v in range(2)]) for r in range(2)]) for j in range(3))


def _views(sel, which):
    """the cameras of the rooms ``sel``, views ``which``"""
    return tuple(x[list(sel)][:, list(which)].contiguous() for x in _cameras())


@functools.lru_cache(maxsize=None)
def _run(sel=(0, 1), which=None, capture=False, mask=None, no_argument=False, **kw):
    """one deterministic RefineBatch run of the rooms ``sel`` with the views ``which`` (None: ``views=None``) -> dict of host arrays.
    ``mask``: None, or per view 0 / 1 - a uint8 mask tensor [R, V, S, S] of all zeros / all ones per view"""
    R, L = pkg("host.refine"), pkg("_lib").lib()
    model, _, rooms, bank = _setup()
    if not no_argument:
        kw["views"] = None if which is None else _views(sel, which)
    if mask is not None:
        kw["mask"] = torch.tensor(mask, dtype=torch.uint8, device="cuda")[None, :, None, None].expand(len(sel), len(mask), IMAGE, IMAGE).contiguous()
    L.sln_set_deterministic(1)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            rb = R.RefineBatch(model, [rooms[i] for i in sel], bank=bank, learning_rate=1e-3, image_size=IMAGE, iters=ITERS, **kw)
            rb.run(capture=capture)
            cpu = lambda t: None if t is None else t.cpu().numpy().copy()
            out = dict(losses=cpu(rb.losses), boxes=[cpu(b) for b, _ in rb.results()], idx=[cpu(i) for _, i in rb.results()], z=cpu(rb.z),
                       params=cpu(rb.params), overlap=cpu(rb.overlap), fused_head=rb._fused_head, row0=rb.row0, rows=rb.rows,
                       mask_status=cpu(rb.mask_status), images=tuple(rb.image.shape), V=rb.V)
            rb.close()
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    return out


def test_views_none_changes_nothing():
    plain, none = _run(no_argument=True), _run()
    assert plain["fused_head"] and none["fused_head"] and none["V"] == 1 and none["images"][0] == 2
    _same_bits(none, plain, "views=None against no argument")


def test_one_view_with_the_refinement_camera_is_the_default_run():
    one, plain = _run(which=(0,)), _run()
    assert not one["fused_head"] and one["V"] == 1 and one["losses"].shape == (ITERS, 2)
    _same_bits(one, plain, "V = 1 with refine_view's camera against the default run")


def test_two_views_rooms_do_not_depend_on_the_batch_and_capture_equals_eager():
    both = _run(which=(0, 1))
    assert both["images"][0] == 4 and both["losses"].shape == (ITERS, 2) and np.isfinite(both["losses"]).all()
    for r in (0, 1):
        _same_bits(_run(sel=(r,), which=(0, 1)), both, "R = 1 (room %d) against R = 2" % r, (0,), (r,))
    _same_bits(_run(which=(0, 1), capture=True), both, "capture against eager")


def test_two_views_with_the_overlap_penalty():
    on, off = _run(which=(0, 1), overlap_weight=WEIGHT), _run(which=(0, 1))
    assert on["overlap"].shape == (ITERS, 2) and (on["overlap"][0] > 0).all(), "the iterates do not interpenetrate: this test shows nothing"
    rest = on["losses"] - (WEIGHT * on["overlap"]).astype(np.float32)
    assert_close(rest[0], off["losses"][0], "iteration 0: the same layout, the loss without its penalty term", rtol=1e-5)
    assert not np.array_equal(on["z"], off["z"])
    for r in (0, 1):
        one = _run(sel=(r,), which=(0, 1), overlap_weight=WEIGHT)
        _same_bits(one, on, "R = 1 (room %d) against R = 2, penalty on" % r, (0,), (r,))
        assert np.array_equal(one["overlap"][:, 0], on["overlap"][:, r])
    _same_bits(_run(which=(0, 1), capture=True, overlap_weight=WEIGHT), on, "capture against eager, penalty on")


def test_two_views_first_loss_is_the_mean_and_the_second_view_reaches_z():
    both, first, second = _run(which=(0, 1)), _run(which=(0,)), _run(which=(1,))
    print("losses, V = 2:\n%s\nview 0 alone:\n%s\nview 1 alone:\n%s" % (both["losses"], first["losses"], second["losses"]))
    # iteration 0: the same z, parameters and noise in all three runs and a size loss of exactly 0 - the loss is the mean of the views'
    assert_close(both["losses"][0], (first["losses"][0].astype(np.float64) + second["losses"][0]) / 2, "losses[0] against the mean of the V = 1 runs",
                 rtol=1e-5)
    assert (np.abs(first["losses"][0] - second["losses"][0]) > 1e-3 * np.abs(first["losses"][0])).all(), "the two views show the same: this test shows nothing"
    for k in range(1, ITERS):
        assert (both["losses"][k] != first["losses"][k]).all(), "iteration %d" % k
    assert not np.array_equal(both["z"], first["z"]) and not np.array_equal(both["z"], second["z"])


def test_two_views_against_the_autograd_loop():
    R, M = pkg("host.refine"), pkg("host.Sg2ScVAE_model")
    _, sd, rooms, bank = _setup()
    batch = _run(which=(0, 1))
    with torch.cuda.stream(torch.cuda.Stream()):
        for r, rm in enumerate(rooms):
            args = (rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"])
            m2 = M.Sg2ScVAEModel(**CFG.model_kwargs()); m2.load_state_dict(sd); m2 = m2.cuda().eval()
            l2, (b2, i2) = R.finetune_vae(m2, *args, iters=ITERS, bank=bank, learning_rate=1e-3, image_size=IMAGE,
                                          views=tuple(x[0] for x in _views((r,), (0, 1))))
            print("room %d: RefineBatch %s, finetune_vae %s" % (r, batch["losses"][:, r], np.asarray(l2)))
            assert_close(batch["losses"][:, r], np.asarray(l2), "losses of room %d vs finetune_vae" % r, rtol=2e-3)
            assert_close(batch["boxes"][r], b2.cpu().numpy(), "boxes of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-4)
            assert_close(batch["params"][r], m2.flat_params.detach().cpu().numpy(), "parameters of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-5)
    torch.cuda.synchronize()


def test_a_missing_view_is_an_all_zero_mask_and_the_divisor_stays():
    half, one = _run(which=(0, 1), mask=(1, 0)), _run(which=(0,), mask=(1,))
    print("mask_status %s, losses[0] %s against the one-view masked run's %s" % (half["mask_status"].tolist(), half["losses"][0], one["losses"][0]))
    assert half["mask_status"].shape == (2, 2) and one["mask_status"].shape == (2, 1)
    assert (half["mask_status"][:, 1] & 3 == 3).all() and (half["mask_status"][:, 0] == 0).all() and (one["mask_status"] == 0).all()
    assert_close(half["losses"][0], one["losses"][0].astype(np.float64) / 2, "losses[0]: half the one-view masked run's", rtol=1e-5)
    assert np.isfinite(half["losses"]).all()


def test_observed_frames_per_view_are_one_target_call_over_all_images():
    """``observed`` [R, V, S, S] - here every view's own render, observed - goes through ONE ObservedTarget call with batch = R * V, image
    b = r * V + v; ``target_status`` and ``mask_status`` come back as [R, V]"""
    R, OB = pkg("host.refine"), pkg("host.observe")
    model, _, rooms, bank = _setup()
    K, Rm, t = _cameras()
    with torch.no_grad():
        render = torch.cat([R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), IMAGE).with_view(K[r, v], Rm[r, v], t[r, v])
                            .render(rm["boxes"], rm["angles"].float())[0] for r, rm in enumerate(rooms) for v in range(2)], 0)
    depth, labels = OB.observe(render)
    obs = (depth.view(2, 2, IMAGE, IMAGE), labels.view(2, 2, IMAGE, IMAGE))
    rb = R.RefineBatch(model, rooms, bank=bank, learning_rate=1e-3, image_size=IMAGE, iters=ITERS, views=(K, Rm, t), observed=obs, mask="readings")
    try:
        target, status = OB.ObservedTarget(rb.chan, rb.dch, IMAGE, batch=4)(depth, labels)
        rl = R.RefineLoss(target, per_room=True, valid=(target[:, 0] >= 0).to(torch.uint8))
        torch.cuda.synchronize()
        assert torch.equal(rb.loss.target_depth.view(torch.int32), rl.target_depth.view(torch.int32)) and torch.equal(rb.loss.labels, rl.labels)
        assert tuple(rb.target_status.shape) == (2, 2) and torch.equal(rb.target_status.reshape(-1), status)
        assert tuple(rb.mask_status.shape) == (2, 2) and torch.equal(rb.mask_status.reshape(-1), rl.mask_status)
        losses = rb.run().cpu().numpy()
        print("losses towards the observed views:\n%s" % losses)
        assert losses.shape == (ITERS, 2) and np.isfinite(losses).all()
    finally:
        rb.close()


def test_refusals():
    R = pkg("host.refine")
    model, _, rooms, bank = _setup()
    kw = dict(bank=bank, image_size=IMAGE, iters=ITERS)
    K, Rm, t = _cameras()
    for extra in (dict(report="ends"), dict(pictures="ends"), dict(retrieve=True)):
        with pytest.raises(ValueError, match="does not combine"):
            R.RefineBatch(model, rooms, views=(K, Rm, t), **extra, **kw)
    with pytest.raises(ValueError, match="views"):
        R.RefineBatch(model, rooms, views=(K[:1], Rm[:1], t[:1]), **kw)
    with pytest.raises(ValueError, match="views"):
        R.RefineBatch(model, rooms, views=(K, Rm, t[..., :2]), **kw)
    with pytest.raises(ValueError, match="at most 64"):
        R.RefineBatch(model, rooms, views=tuple(x[:, :1].repeat_interleave(65, 1) for x in (K, Rm, t)), **kw)
    bad = t.clone(); bad[1, 0, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        R.RefineBatch(model, rooms, views=(K, Rm, bad), **kw)
    u8 = dict(dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="V axis"):
        R.RefineBatch(model, rooms, views=(K, Rm, t), mask=torch.ones(2, IMAGE, IMAGE, **u8), **kw)
    with pytest.raises(ValueError, match="V axis"):
        R.RefineBatch(model, rooms, views=(K, Rm, t), observed=(torch.ones(2, IMAGE, IMAGE, device="cuda"), torch.ones(2, IMAGE, IMAGE, **u8)), **kw)
    with pytest.raises(ValueError, match="does not combine"):
        R.finetune_vae_fast_batch(model, rooms, views=(K, Rm, t), report="all", **kw)
    rm = rooms[0]
    with pytest.raises(ValueError, match="views"):
        R.finetune_vae(model, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=1, bank=bank,
                       image_size=IMAGE, views=(K, Rm, t))                      # the one-room form has no room axis
    # without views the mask keeps its shape [R, S, S]
    with pytest.raises(ValueError, match="mask"):
        R.RefineBatch(model, rooms, mask=torch.ones(2, 2, IMAGE, IMAGE, **u8), **kw)
