"""Refinement of the camera poses of the target views inside the refinement loops (``poses=`` of RefineBatch, finetune_vae_fast_batch and
finetune_vae; DESIGN §4 "Camera poses of the target views"): the set-up of tests/test_refine_views_gpu.py - its two rooms at 64 x 64, its two
views per room, four iterations, deterministic mode.  In the runs that step, the loop starts from the target cameras with view 1 turned by
0.02 rad and moved by 0.02.  No convergence is asserted: the rasterised loss is not smooth."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

from test_refine_overlap_gpu import CFG, IMAGE, ITERS, _same_bits, _setup
import test_refine_views_gpu as TV

pytestmark = pytest.mark.gpu

# the entries of d omega and d tau of these rooms are of the order 0.1 - 2 (LAB_NOTES §42): steps that move a pose by a few 1e-5 rad / 1e-5 per
# iteration - 1.6e-4 in R and 9.5e-4 in t over the four iterations, well above the float32 rounding of the table (6e-8, 5e-7) and small
# against the 0.02 perturbation.  Measured against the yardstick: max |d R| 2.9e-8, max |d t| 1.5e-7 - no silhouette noise to allow for.
ROT_STEP, TRANS_STEP = 2e-5, 2e-5


@functools.lru_cache(maxsize=None)
def _start(sel=(0, 1)):
    """(Rm [R, 2, 3, 3], t [R, 2, 3]) float64: the target cameras of the rooms ``sel`` with view 1 turned by 0.02 rad and moved by 0.02"""
    RP = pkg("host.reproject")
    _, Rm, t = TV._views(sel, (0, 1))
    Rm, t = Rm.double().clone(), t.double().clone()
    om = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64) * 0.02
    ta = torch.tensor([-0.48, 0.64, 0.6], dtype=torch.float64) * 0.02
    Rm[:, 1], t[:, 1] = RP.pose_step_torch(Rm[:, 1], t[:, 1], om, ta)
    return Rm, t


def _poses(sel, steps, free=None, start=True):
    if steps is None:
        return None
    p = dict(rot_step=steps[0], trans_step=steps[1])
    if start:
        p["start"] = _start(sel)
    if free is not None:
        p["free"] = torch.tensor(free, dtype=torch.bool)[None].expand(len(sel), 2).contiguous()
    return p


@functools.lru_cache(maxsize=None)
def _run(sel=(0, 1), steps=None, capture=False, free=None, start=True, no_argument=False, record=False):
    """one deterministic RefineBatch run of the rooms ``sel`` against views (0, 1); ``steps``: None (``poses=None``) or (rot_step, trans_step)
    -> dict of host arrays; ``record``: with ``calls``, the library calls of ``run()`` in order (tests/test_refine_sequence_gpu.py's proxy)"""
    R, Lm = pkg("host.refine"), pkg("_lib")
    L = Lm.lib()
    model, _, rooms, bank = _setup()
    kw = {} if no_argument else dict(poses=_poses(sel, steps, free, start))
    L.sln_set_deterministic(1)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            rb = R.RefineBatch(model, [rooms[i] for i in sel], bank=bank, learning_rate=1e-3, image_size=IMAGE, iters=ITERS, views=TV._views(sel, (0, 1)), **kw)
            cams0 = rb._cams.clone()
            calls = None
            if record:
                Lm._lib = proxy = _Ordered(L)
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
                       pose_grad=None, poses=None)
            if steps is not None:
                out.update(pose_grad=cpu(rb.pose_grad), poses=tuple(cpu(x) for x in rb.poses()),
                           error=tuple(cpu(x) for x in rb.pose_error(*(x[list(sel)][:, [0, 1]] for x in TV._cameras()[1:]))))
            rb.close()
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    return out


class _Ordered:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


def _same_poses(a, b, what, rooms_a=(0, 1), rooms_b=(0, 1)):
    for ja, jb in zip(rooms_a, rooms_b):
        assert np.array_equal(a["pose_grad"][:, ja], b["pose_grad"][:, jb]), "%s: pose gradients" % what
        assert all(np.array_equal(x[ja], y[jb]) for x, y in zip(a["poses"], b["poses"])), "%s: poses" % what
        assert np.array_equal(a["cams"].reshape(-1, 2, 21)[ja], b["cams"].reshape(-1, 2, 21)[jb]), "%s: camera table" % what


def test_poses_none_changes_nothing():
    plain, none = _run(no_argument=True, record=True), _run(record=True)
    _same_bits(none, plain, "poses=None against no argument")
    _same_bits(none, TV._run(which=(0, 1)), "poses=None against the views run")
    assert none["calls"] == plain["calls"] and "sln_place_pose_step_views" not in none["calls"]
    assert none["calls"].count("sln_place_backward_views") == ITERS
    assert np.array_equal(none["cams"], none["cams0"]), "the camera table is not the one uploaded at set-up"
    # with poses: the same calls with the one launch behind every placement backward
    want = []
    for name in plain["calls"]:
        want += [name, "sln_place_pose_step_views"] if name == "sln_place_backward_views" else [name]
    assert _run(steps=(0.0, 0.0), start=False, record=True)["calls"] == want


def test_steps_zero_record_the_gradients_and_change_nothing():
    zero, plain = _run(steps=(0.0, 0.0), start=False), _run()
    _same_bits(zero, plain, "both steps 0 against poses=None")
    assert np.array_equal(zero["cams"], zero["cams0"]) and np.array_equal(zero["cams"], plain["cams"]), "steps 0: the camera table moved"
    g = zero["pose_grad"]
    print("pose_grad [iters, R, V, 6] at steps 0:\n%s" % np.array2string(g, precision=4))
    assert g.shape == (ITERS, 2, 2, 6) and g.dtype == np.float64 and np.isfinite(g).all()
    assert (np.abs(g).max(-1) > 0).all(), "a (room, view) without a pose gradient"
    Rm, t = zero["poses"]
    assert np.array_equal(Rm.reshape(4, 9), zero["cams0"][:, 9:18].astype(np.float64)) and np.array_equal(t.reshape(4, 3), zero["cams0"][:, 18:].astype(np.float64))
    assert (zero["error"][0] == 0).all() and (zero["error"][1] == 0).all()


def test_steps_move_the_poses_rooms_do_not_depend_on_the_batch_and_capture_equals_eager():
    both, still = _run(steps=(ROT_STEP, TRANS_STEP)), _run(steps=(0.0, 0.0))
    print("losses with the steps on:\n%s\nat steps 0 from the same start:\n%s\npose error (rad, distance) after %d iterations: %s, at the start: %s" %
          (both["losses"], still["losses"], ITERS, both["error"], still["error"]))
    assert np.isfinite(both["losses"]).all() and np.isfinite(both["poses"][0]).all()
    assert np.array_equal(both["losses"][0], still["losses"][0]) and (both["losses"][1:] != still["losses"][1:]).all()
    assert abs(still["error"][0][:, 1] - 0.02).max() <= 1e-6 and abs(still["error"][1][:, 1] - 0.02).max() <= 1e-6 and (still["error"][0][:, 0] <= 1e-6).all()
    moved = np.abs(both["cams"] - both["cams0"]).reshape(2, 2, 21)
    assert (moved[..., :9] == 0).all(), "K was written"
    assert (moved[..., 9:].max(-1) > 0).all(), "a free view whose table entry did not move"
    assert np.array_equal(both["cams"][:, 9:], np.concatenate([x.reshape(4, -1) for x in both["poses"]], 1).astype(np.float32)), "table != float32(master)"
    for r in (0, 1):
        one = _run(sel=(r,), steps=(ROT_STEP, TRANS_STEP))
        _same_bits(one, both, "R = 1 (room %d) against R = 2" % r, (0,), (r,))
        _same_poses(one, both, "R = 1 (room %d) against R = 2" % r, (0,), (r,))
    graph = _run(steps=(ROT_STEP, TRANS_STEP), capture=True)
    _same_bits(graph, both, "capture against eager")
    _same_poses(graph, both, "capture against eager")


def test_a_view_that_is_not_free_keeps_its_table_row():
    held, both = _run(steps=(ROT_STEP, TRANS_STEP), free=(False, True)), _run(steps=(ROT_STEP, TRANS_STEP))
    cams, cams0 = held["cams"].reshape(2, 2, 21), held["cams0"].reshape(2, 2, 21)
    assert np.array_equal(cams[:, 0].view(np.int32), cams0[:, 0].view(np.int32)), "view 0 is held: its table row was written"
    assert (np.abs(cams[:, 1] - cams0[:, 1])[:, 9:].max(-1) > 0).all()
    assert (np.abs(held["pose_grad"][:, :, 0]).max(-1) > 0).all(), "the held view's gradient is still recorded"
    assert np.array_equal(held["pose_grad"][0], both["pose_grad"][0]) and not np.array_equal(held["losses"][1:], both["losses"][1:])


def _yardstick(r):
    """finetune_vae(views=, poses=) of room r -> (losses, boxes, idx, parameters, Rm, t)"""
    R, M = pkg("host.refine"), pkg("host.Sg2ScVAE_model")
    _, sd, rooms, bank = _setup()
    rm = rooms[r]
    with torch.cuda.stream(torch.cuda.Stream()):
        m2 = M.Sg2ScVAEModel(**CFG.model_kwargs()); m2.load_state_dict(sd); m2 = m2.cuda().eval()
        l2, (b2, i2), (Rm, t) = R.finetune_vae(m2, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=ITERS,
                                               bank=bank, learning_rate=1e-3, image_size=IMAGE, views=tuple(x[0] for x in TV._views((r,), (0, 1))),
                                               poses=dict(rot_step=ROT_STEP, trans_step=TRANS_STEP, start=tuple(x[0] for x in _start((r,)))))
        out = (np.asarray(l2), b2.cpu().numpy(), i2.cpu().numpy(), m2.flat_params.detach().cpu().numpy(), Rm.numpy(), t.numpy())
    torch.cuda.synchronize()
    return out


def test_against_the_autograd_loop():
    """losses, boxes and parameters at the tolerances of tests/test_refine_views_gpu.py::test_two_views_against_the_autograd_loop, the angles at
    the boxes'; the poses within 1e-4 (rotation entries) and 1e-4 of the room's extent (t)"""
    _, _, rooms, _ = _setup()
    batch = _run(steps=(ROT_STEP, TRANS_STEP))
    for r, rm in enumerate(rooms):
        l2, b2, i2, p2, Rm, t = _yardstick(r)
        ext = float(rm["boxes"][-1, 3:].max())
        dR, dt = np.abs(batch["poses"][0][r] - Rm).max(), np.abs(batch["poses"][1][r] - t).max()
        s0 = _start((r,))
        print("room %d: RefineBatch %s, finetune_vae %s; poses: max |d R| = %.3e, max |d t| = %.3e (extent %.2f); moved from the start by %.3e / %.3e" %
              (r, batch["losses"][:, r], l2, dR, dt, ext, np.abs(Rm - s0[0][0].numpy()).max(), np.abs(t - s0[1][0].numpy()).max()))
        assert_close(batch["losses"][:, r], l2, "losses of room %d vs finetune_vae" % r, rtol=2e-3)
        assert_close(batch["boxes"][r], b2, "boxes of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-4)
        assert_close(batch["idx"][r], i2, "angles of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-4)
        assert_close(batch["params"][r], p2, "parameters of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-5)
        assert dR <= 1e-4 and dt <= 1e-4 * ext, "poses of room %d vs finetune_vae" % r


def test_refusals():
    R = pkg("host.refine")
    model, _, rooms, bank = _setup()
    kw = dict(bank=bank, image_size=IMAGE, iters=ITERS)
    views = TV._views((0, 1), (0, 1))
    ok = dict(rot_step=1e-5, trans_step=1e-5)
    with pytest.raises(ValueError, match="needs views"):
        R.RefineBatch(model, rooms, poses=ok, **kw)
    with pytest.raises(ValueError, match="unknown keys"):
        R.RefineBatch(model, rooms, views=views, poses=dict(ok, lr=1.0), **kw)
    with pytest.raises(ValueError, match="rot_step"):
        R.RefineBatch(model, rooms, views=views, poses=dict(ok, rot_step=-1.0), **kw)
    with pytest.raises(ValueError, match="trans_step"):
        R.RefineBatch(model, rooms, views=views, poses=dict(ok, trans_step=float("inf")), **kw)
    with pytest.raises(ValueError, match="free"):
        R.RefineBatch(model, rooms, views=views, poses=dict(ok, free=torch.ones(2, 3, dtype=torch.bool)), **kw)
    with pytest.raises(ValueError, match="start"):
        R.RefineBatch(model, rooms, views=views, poses=dict(ok, start=(views[1][:1], views[2][:1])), **kw)
    with pytest.raises(ValueError, match="orthonormal"):
        R.RefineBatch(model, rooms, views=views, poses=dict(ok, start=(views[1] * 1.001, views[2])), **kw)
    with pytest.raises(ValueError, match="needs views"):
        R.finetune_vae_fast_batch(model, rooms, poses=ok, **kw)
    rm = rooms[0]
    with pytest.raises(ValueError, match="needs views"):
        R.finetune_vae(model, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=1, bank=bank,
                       image_size=IMAGE, poses=ok)
