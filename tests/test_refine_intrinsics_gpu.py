"""Refinement of the intrinsics of the target views inside the refinement loops (``intrinsics=`` of RefineBatch, finetune_vae_fast_batch and
finetune_vae; DESIGN §4 "Intrinsics of the target views"): the set-up of tests/test_refine_poses_gpu.py - its two rooms at 64 x 64, its two
views per room, four iterations, deterministic mode.  In the runs that step, the loop starts from the target cameras with the focal lengths
of view 1 3 % high.  One descent is asserted, of the focal error of that view with the poses exact and held; nothing else about convergence:
the rasterised loss is not smooth."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

from test_refine_overlap_gpu import CFG, IMAGE, ITERS, _same_bits, _setup
import test_refine_poses_gpu as TPo
import test_refine_views_gpu as TV

pytestmark = pytest.mark.gpu

# fx dL/dfx of these rooms is of the order 0.1 - 3, dL/dcx of the order 0.01 - 0.1 (the steps-0 test prints them): a focal step that scales a
# focal length by a few 1e-4 - 1e-3 per iteration and a centre step that moves the principal point by a few 1e-3 - 1e-2 pixels of
# orig_size = 512 - well above the float32 rounding of the table (1.5e-5 at 200, 3e-5 at 256) and small against the 3 % = 6 pixels of the start
FOCAL_STEP, CENTER_STEP = 1e-3, 0.1
STEPS = (FOCAL_STEP, CENTER_STEP)
HIGH = 1.03


@functools.lru_cache(maxsize=None)
def _start(sel=(0, 1)):
    """K [R, 2, 3, 3] float64: the target K of the rooms ``sel`` with fx, fy of view 1 3 % high"""
    K = TV._views(sel, (0, 1))[0].double().clone()
    K[:, 1, 0, 0] *= HIGH
    K[:, 1, 1, 1] *= HIGH
    return K


def _intrinsics(sel, steps, tie=True, free=None, start=True):
    if steps is None:
        return None
    p = dict(focal_step=steps[0], center_step=steps[1], tie_focal=tie)
    if start:
        p["start"] = _start(sel)
    if free is not None:
        p["free"] = torch.tensor(free, dtype=torch.bool)[None].expand(len(sel), 2).contiguous()
    return p


@functools.lru_cache(maxsize=None)
def _run(sel=(0, 1), steps=None, pose_steps=None, capture=False, tie=True, free=None, start=True, record=False):
    """one deterministic RefineBatch run of the rooms ``sel`` against views (0, 1); ``steps``: None (``intrinsics=None``) or (focal_step,
    center_step); ``pose_steps``: None (``poses=None``) or (rot_step, trans_step) from tests/test_refine_poses_gpu.py's perturbed start
    -> dict of host arrays; ``record``: with ``calls``, the library calls of ``run()`` in order"""
    R, Lm = pkg("host.refine"), pkg("_lib")
    L = Lm.lib()
    model, _, rooms, bank = _setup()
    L.sln_set_deterministic(1)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            rb = R.RefineBatch(model, [rooms[i] for i in sel], bank=bank, learning_rate=1e-3, image_size=IMAGE, iters=ITERS, views=TV._views(sel, (0, 1)),
                               poses=TPo._poses(sel, pose_steps), intrinsics=_intrinsics(sel, steps, tie, free, start))
            cams0 = rb._cams.clone()
            calls = None
            if record:
                Lm._lib = proxy = TPo._Ordered(L)
                try:
                    rb.run(capture=capture)
                finally:
                    Lm._lib = L
                calls = list(proxy.calls)
            else:
                rb.run(capture=capture)
            cpu = lambda t: None if t is None else t.cpu().numpy().copy()
            out = dict(losses=cpu(rb.losses), boxes=[cpu(b) for b, _ in rb.results()], idx=[cpu(i) for _, i in rb.results()], z=cpu(rb.z),
                       params=cpu(rb.params), row0=rb.row0, rows=rb.rows, cams0=cpu(cams0), cams=cpu(rb._cams), calls=calls,
                       pose_grad=None, poses=None, intr_grad=None, K=None)
            if steps is not None or pose_steps is not None:
                out.update(pose_grad=cpu(rb.pose_grad), poses=tuple(cpu(x) for x in rb.poses()))
            if steps is not None:
                K_ref = TV._views(sel, (0, 1))[0]
                out.update(intr_grad=cpu(rb.intr_grad), K=cpu(rb.intrinsics()), error=tuple(cpu(x) for x in rb.intrinsics_error(K_ref)))
            rb.close()
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    return out


def _same_camera(a, b, what, rooms_a=(0, 1), rooms_b=(0, 1)):
    for ja, jb in zip(rooms_a, rooms_b):
        assert np.array_equal(a["intr_grad"][:, ja], b["intr_grad"][:, jb]), "%s: gradients of the intrinsics" % what
        assert np.array_equal(a["pose_grad"][:, ja], b["pose_grad"][:, jb]), "%s: pose gradients" % what
        assert np.array_equal(a["K"][ja], b["K"][jb]), "%s: K" % what
        assert np.array_equal(a["cams"].reshape(-1, 2, 21)[ja], b["cams"].reshape(-1, 2, 21)[jb]), "%s: camera table" % what


def test_intrinsics_none_changes_nothing_with_and_without_poses():
    pose_steps = (TPo.ROT_STEP, TPo.TRANS_STEP)
    for ps in (None, pose_steps):
        today, none = TPo._run(steps=ps, record=True), _run(pose_steps=ps, record=True)
        _same_bits(none, today, "intrinsics=None against a run without the argument (poses %s)" % (ps,))
        assert none["calls"] == today["calls"] and "sln_place_camera_step_views" not in none["calls"]
        assert np.array_equal(none["cams"], today["cams"])
        if ps is not None:
            TPo._same_poses(none, today, "intrinsics=None, poses on")
            assert none["calls"].count("sln_place_pose_step_views") == ITERS
        # with intrinsics: the new launch in the place of the pose launch / behind every placement backward - one launch, never two
        want = []
        for name in TPo._run(record=True)["calls"]:
            want += [name, "sln_place_camera_step_views"] if name == "sln_place_backward_views" else [name]
        got = _run(steps=(0.0, 0.0), pose_steps=ps, start=False, record=True)["calls"]
        assert got == want and "sln_place_pose_step_views" not in got


def test_steps_zero_record_the_gradients_and_change_nothing():
    zero, plain = _run(steps=(0.0, 0.0), start=False), TPo._run()
    _same_bits(zero, plain, "both steps 0 against intrinsics=None")
    assert np.array_equal(zero["cams"], zero["cams0"]) and np.array_equal(zero["cams"], plain["cams"]), "steps 0: the camera table moved"
    g = zero["intr_grad"]
    print("intr_grad [iters, R, V, 4] = (d fx, d fy, d cx, d cy) at steps 0:\n%s\nfx d fx, fy d fy:\n%s" %
          (np.array2string(g, precision=5), np.array2string(g[..., :2] * zero["K"][:, :, [0, 1], [0, 1]], precision=4)))
    assert g.shape == (ITERS, 2, 2, 4) and g.dtype == np.float64 and np.isfinite(g).all()
    assert (np.abs(g).max(-1) > 0).all(), "a (room, view) without a gradient"
    assert np.array_equal(zero["pose_grad"], TPo._run(steps=(0.0, 0.0), start=False)["pose_grad"]), "pose_grad is recorded as the pose launch records it"
    K = zero["K"]
    assert K.dtype == np.float64 and np.array_equal(K.reshape(4, 9), zero["cams0"][:, :9].astype(np.float64))
    assert (zero["error"][0] == 0).all() and (zero["error"][1] == 0).all()


def test_steps_move_K_rooms_do_not_depend_on_the_batch_and_capture_equals_eager():
    both, still = _run(steps=STEPS), _run(steps=(0.0, 0.0))
    print("losses with the steps on:\n%s\nat steps 0 from the same start:\n%s\nerror (relative focal, centre in pixels) after %d iterations: %s, at the start: %s" %
          (both["losses"], still["losses"], ITERS, both["error"], still["error"]))
    assert np.isfinite(both["losses"]).all() and np.isfinite(both["K"]).all()
    assert np.array_equal(both["losses"][0], still["losses"][0]) and (both["losses"][1:] != still["losses"][1:]).all()
    assert abs(still["error"][0][:, 1] - (HIGH - 1)).max() <= 1e-6 and (still["error"][0][:, 0] == 0).all() and (still["error"][1] == 0).all()
    moved = np.abs(both["cams"] - both["cams0"]).reshape(2, 2, 21)
    assert (moved[..., 9:] == 0).all(), "R or t was written with poses=None"
    assert (moved[..., [1, 3, 6, 7, 8]] == 0).all(), "the skew entries or the last row of K were written"
    assert (moved[..., [0, 4, 2, 5]] > 0).all(), "a free view whose fx, fy, cx or cy did not move"
    assert np.array_equal(both["cams"][:, :9], both["K"].reshape(4, 9).astype(np.float32)), "table != float32(master)"
    ratio, ratio0 = both["K"][..., 0, 0] / both["K"][..., 1, 1], (both["cams0"][:, 0].astype(np.float64) / both["cams0"][:, 4]).reshape(2, 2)
    assert (np.abs(ratio - ratio0) <= 5 * 2.0 ** -53 * ITERS * ratio0).all(), "tie_focal: the aspect ratio moved by more than the rounding of four steps"
    for r in (0, 1):
        one = _run(sel=(r,), steps=STEPS)
        _same_bits(one, both, "R = 1 (room %d) against R = 2" % r, (0,), (r,))
        _same_camera(one, both, "R = 1 (room %d) against R = 2" % r, (0,), (r,))
    graph = _run(steps=STEPS, capture=True)
    _same_bits(graph, both, "capture against eager")
    _same_camera(graph, both, "capture against eager")
    untied = _run(steps=STEPS, tie=False)
    assert not np.array_equal(untied["K"], both["K"]) and np.array_equal(untied["intr_grad"][0], both["intr_grad"][0])


def test_a_view_that_is_not_free_keeps_its_K():
    held, both = _run(steps=STEPS, free=(False, True)), _run(steps=STEPS)
    cams, cams0 = held["cams"].reshape(2, 2, 21), held["cams0"].reshape(2, 2, 21)
    assert np.array_equal(cams[:, 0].view(np.int32), cams0[:, 0].view(np.int32)), "view 0 is held: its table row was written"
    assert np.array_equal(held["K"][:, 0], cams0[:, 0, :9].reshape(2, 3, 3).astype(np.float64)), "view 0 is held: its master was written"
    assert (np.abs(cams[:, 1] - cams0[:, 1])[:, [0, 4, 2, 5]] > 0).all()
    assert (np.abs(held["intr_grad"][:, :, 0]).max(-1) > 0).all(), "the held view's gradient is still recorded"
    assert np.array_equal(held["intr_grad"][0], both["intr_grad"][0]) and not np.array_equal(held["losses"][1:], both["losses"][1:])


def test_intrinsics_together_with_poses():
    pose_steps = (TPo.ROT_STEP, TPo.TRANS_STEP)
    both, pose, intr = _run(steps=STEPS, pose_steps=pose_steps), _run(steps=(0.0, 0.0), pose_steps=pose_steps), _run(steps=STEPS, pose_steps=(0.0, 0.0))
    assert np.isfinite(both["losses"]).all() and np.isfinite(both["K"]).all() and np.isfinite(both["poses"][0]).all()
    # iteration 0 sees the same start in all three: one pair of gradients by bits, and each half steps as it does alone
    for key in ("pose_grad", "intr_grad"):
        assert np.array_equal(both[key][0], pose[key][0]) and np.array_equal(both[key][0], intr[key][0]), key
    assert not np.array_equal(both["losses"][1:], pose["losses"][1:]) and not np.array_equal(both["losses"][1:], intr["losses"][1:])
    moved = np.abs(both["cams"] - both["cams0"]).reshape(2, 2, 21)
    assert (moved[..., [0, 4, 2, 5]] > 0).all() and (moved[..., 9:].max(-1) > 0).all() and (moved[..., [1, 3, 6, 7, 8]] == 0).all()
    assert np.array_equal(both["cams"][:, 9:], np.concatenate([x.reshape(4, -1) for x in both["poses"]], 1).astype(np.float32))
    assert np.array_equal(both["cams"][:, :9], both["K"].reshape(4, 9).astype(np.float32))
    # the pose half at intrinsics steps 0 is the pose loop of before, by bits
    today, exact = TPo._run(steps=pose_steps), _run(steps=(0.0, 0.0), pose_steps=pose_steps, start=False)       # (the K of the views: today's start)
    _same_bits(exact, today, "poses with intrinsics at steps 0 against poses alone")
    TPo._same_poses(exact, today, "poses with intrinsics at steps 0 against poses alone")
    graph = _run(steps=STEPS, pose_steps=pose_steps, capture=True)
    _same_bits(graph, both, "capture against eager")
    _same_camera(graph, both, "capture against eager")
    TPo._same_poses(graph, both, "capture against eager")


def _yardstick(r, pose_steps=None):
    """finetune_vae(views=, intrinsics=) of room r -> (losses, boxes, idx, parameters, K)"""
    R, M = pkg("host.refine"), pkg("host.Sg2ScVAE_model")
    _, sd, rooms, bank = _setup()
    rm = rooms[r]
    with torch.cuda.stream(torch.cuda.Stream()):
        m2 = M.Sg2ScVAEModel(**CFG.model_kwargs()); m2.load_state_dict(sd); m2 = m2.cuda().eval()
        poses = None if pose_steps is None else dict(rot_step=pose_steps[0], trans_step=pose_steps[1], start=tuple(x[0] for x in TPo._start((r,))))
        res = R.finetune_vae(m2, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=ITERS,
                             bank=bank, learning_rate=1e-3, image_size=IMAGE, views=tuple(x[0] for x in TV._views((r,), (0, 1))), poses=poses,
                             intrinsics=dict(focal_step=FOCAL_STEP, center_step=CENTER_STEP, start=_start((r,))[0]))
        out = (np.asarray(res[0]), res[1][0].cpu().numpy(), res[1][1].cpu().numpy(), m2.flat_params.detach().cpu().numpy(), res[-1].numpy())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("with_poses", [False, True], ids=["alone", "with-poses"])
def test_against_the_autograd_loop(with_poses):
    """losses, boxes and parameters at the tolerances of tests/test_refine_views_gpu.py::test_two_views_against_the_autograd_loop, the angles at
    the boxes'; how closely K agrees is printed, and held to a twentieth of what the loop moved it by"""
    _, _, rooms, _ = _setup()
    pose_steps = (TPo.ROT_STEP, TPo.TRANS_STEP) if with_poses else None
    batch = _run(steps=STEPS, pose_steps=pose_steps)
    for r, rm in enumerate(rooms):
        l2, b2, i2, p2, K = _yardstick(r, pose_steps)
        s0 = _start((r,))[0].numpy()
        d, moved = np.abs(batch["K"][r] - K), np.abs(K - s0)
        print("room %d: RefineBatch %s, finetune_vae %s\n   K: max |RefineBatch - finetune_vae| = %.3e (focal) %.3e (centre); moved from the start by %.3e (focal) %.3e "
              "(centre)" % (r, batch["losses"][:, r], l2, d[:, [0, 1], [0, 1]].max(), d[:, :2, 2].max(), moved[:, [0, 1], [0, 1]].max(), moved[:, :2, 2].max()))
        assert_close(batch["losses"][:, r], l2, "losses of room %d vs finetune_vae" % r, rtol=2e-3)
        assert_close(batch["boxes"][r], b2, "boxes of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-4)
        assert_close(batch["idx"][r], i2, "angles of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-4)
        assert_close(batch["params"][r], p2, "parameters of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-5)
        assert d[:, [0, 1], [0, 1]].max() <= 0.05 * moved[:, [0, 1], [0, 1]].max() and d[:, :2, 2].max() <= 0.05 * moved[:, :2, 2].max(), "K of room %d" % r


def test_a_focal_length_started_3_percent_high_comes_down():
    """view 1 starts with fx, fy 3 % high, the poses exact and held (``poses=None``), the principal point held (centre step 0), the focal
    lengths tied: after the four iterations the focal error of view 1 is strictly below its start, in both rooms"""
    run = _run(steps=(FOCAL_STEP, 0.0))
    start = HIGH - 1.0
    err = run["error"][0]
    print("relative focal error [room, view] after %d iterations: %s (view 1 started at %.4f, view 0 exact); fx d fx of view 1 per iteration:\n%s" %
          (ITERS, err, start, run["intr_grad"][:, :, 1, 0] * run["K"][None, :, 1, 0, 0]))
    assert (run["error"][1] == 0).all(), "the principal point moved at centre step 0"
    assert (err[:, 1] < start).all(), "the focal error of view 1 did not fall"


def test_refusals():
    R = pkg("host.refine")
    model, _, rooms, bank = _setup()
    kw = dict(bank=bank, image_size=IMAGE, iters=ITERS)
    views = TV._views((0, 1), (0, 1))
    ok = dict(focal_step=1e-3, center_step=0.1)
    with pytest.raises(ValueError, match="needs views"):
        R.RefineBatch(model, rooms, intrinsics=ok, **kw)
    with pytest.raises(ValueError, match="unknown keys"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, lr=1.0), **kw)
    with pytest.raises(ValueError, match="focal_step"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, focal_step=-1.0), **kw)
    with pytest.raises(ValueError, match="center_step"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, center_step=float("inf")), **kw)
    with pytest.raises(ValueError, match="free"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, free=torch.ones(2, 3, dtype=torch.bool)), **kw)
    with pytest.raises(ValueError, match="start"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, start=views[0][:1]), **kw)
    skew = views[0].clone(); skew[0, 1, 0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, start=skew), **kw)
    with pytest.raises(ValueError, match="skew"):
        R.RefineBatch(model, rooms, views=(skew, views[1], views[2]), intrinsics=ok, **kw)
    with pytest.raises(ValueError, match="not positive"):
        R.RefineBatch(model, rooms, views=views, intrinsics=dict(ok, start=-views[0] * torch.tensor([[1.0, 1, 1], [1, 1, 1], [-1, -1, -1]])), **kw)
    with pytest.raises(ValueError, match="needs views"):
        R.finetune_vae_fast_batch(model, rooms, intrinsics=ok, **kw)
    rm = rooms[0]
    with pytest.raises(ValueError, match="needs views"):
        R.finetune_vae(model, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=1, bank=bank,
                       image_size=IMAGE, intrinsics=ok)
    with pytest.raises(ValueError, match="no intrinsics are refined"):
        rb = R.RefineBatch(model, rooms, views=views, **kw)
        try:
            rb.intrinsics()
        finally:
            rb.close()
