"""The interpenetration penalty inside the refinement loops (``overlap_weight`` / ``overlap_rows`` of RefineBatch, finetune_vae_fast and
finetune_vae): two synthetic rooms of tests/test_refine_gpu.py at 64 x 64, four iterations.  The decoder of ``_room_model`` puts every
object into the same corner of the view, so the iterates' furniture interpenetrates from iteration 0 on.  Tolerances between loops are
those tests/test_refine_gpu.py uses for the same pairs of loops without the penalty."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

import test_refine_gpu as TR

pytestmark = pytest.mark.gpu

from oracle import vae_ref     # noqa: E402   (the configs of the fixtures)

IMAGE, ITERS, WEIGHT = 64, 4, 2.0
CFG = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="none", decoder_cat=False)


@functools.lru_cache(maxsize=None)
def _setup():
    R = pkg("host.refine")
    model, sd = TR._room_model(CFG)
    return model, sd, TR._random_rooms(2, CFG, seed=3), R.MeshBank(TR.FURN, "cuda", seed=3)


@functools.lru_cache(maxsize=None)
def _run(sel=(0, 1), capture=False, steps=False, **kw):
    """one deterministic RefineBatch run of the rooms ``sel`` -> dict of host arrays; ``steps``: iteration by iteration, keeping every iterate"""
    R, L = pkg("host.refine"), pkg("_lib").lib()
    model, _, rooms, bank = _setup()
    kw = {k: (v if not isinstance(v, tuple) else [None if x is None else list(x) for x in v]) for k, v in kw.items()}
    L.sln_set_deterministic(1)
    try:
        with torch.cuda.stream(torch.cuda.Stream()):
            rb = R.RefineBatch(model, [rooms[i] for i in sel], bank=bank, learning_rate=1e-3, image_size=IMAGE, iters=ITERS, **kw)
            iterates = []
            if steps:
                for _ in range(ITERS):
                    rb.run(1)
                    iterates.append((rb.boxes.clone(), rb.idx.clone()))
            else:
                rb.run(capture=capture)
            out = dict(losses=rb.losses.cpu().numpy().copy(), boxes=[b.cpu().numpy().copy() for b, _ in rb.results()],
                       idx=[i.cpu().numpy().copy() for _, i in rb.results()], z=rb.z.cpu().numpy().copy(), params=rb.params.cpu().numpy().copy(),
                       overlap=None if rb.overlap is None else rb.overlap.cpu().numpy().copy(), fused_head=rb._fused_head, row0=rb.row0, rows=rb.rows,
                       iterates=iterates, collide=None if rb.overlap is None else rb._collide.clone())
            rb.close()
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    return out


def _same_bits(a, b, what, rooms_a=(0, 1), rooms_b=(0, 1)):
    for ja, jb in zip(rooms_a, rooms_b):
        assert np.array_equal(a["losses"][:, ja], b["losses"][:, jb]), "%s: losses" % what
        assert np.array_equal(a["boxes"][ja], b["boxes"][jb]) and np.array_equal(a["idx"][ja], b["idx"][jb]), "%s: layout" % what
        ra, rb_, n = a["row0"][ja], b["row0"][jb], a["rows"][ja]
        assert np.array_equal(a["z"][ra:ra + n], b["z"][rb_:rb_ + n]), "%s: z" % what
        assert np.array_equal(a["params"][ja], b["params"][jb]), "%s: parameters" % what


def test_weight_zero_changes_nothing():
    plain, zero = _run(), _run(overlap_weight=0.0)
    assert plain["fused_head"] and zero["fused_head"] and zero["overlap"] is None
    _same_bits(zero, plain, "overlap_weight=0.0 against no argument")


def test_penalty_is_recorded_and_reaches_z():
    on, off = _run(overlap_weight=WEIGHT), _run()
    print("overlap per iteration and room:\n%s\nlosses with the weight on:\n%s\nwithout:\n%s" % (on["overlap"], on["losses"], off["losses"]))
    assert not on["fused_head"] and on["overlap"].shape == (ITERS, 2) and on["overlap"].dtype == np.float64
    assert (on["overlap"][0] > 0).all(), "the iterates do not interpenetrate: this file shows nothing"
    rest = on["losses"] - (WEIGHT * on["overlap"]).astype(np.float32)
    assert_close(rest[0], off["losses"][0], "iteration 0: the same layout, the loss without its penalty term", rtol=1e-5)
    for k in range(1, ITERS):
        assert (np.abs(rest[k] - off["losses"][k]) > 1e-4 * np.abs(off["losses"][k])).all(), "iteration %d: the penalty's gradient did not reach z" % k
    assert not np.array_equal(on["z"], off["z"])


def test_recorded_penalty_is_layout_overlap_of_the_iterate():
    EV = pkg("host.evaluate")
    run = _run(steps=True, overlap_weight=WEIGHT)
    _same_bits(run, _run(overlap_weight=WEIGHT), "run(1) four times against run()")
    for k, (boxes, idx) in enumerate(run["iterates"]):
        for r, (a, n) in enumerate(zip(run["row0"], run["rows"])):
            rr = torch.full((n,), n - 1, dtype=torch.int32, device="cuda")
            vol, _ = EV.layout_overlap(boxes[a:a + n][None], idx[a:a + n][None], rr, run["collide"][a:a + n])
            err = abs(float(vol) - run["overlap"][k, r])
            print("iteration %d room %d: overlap %.12g, layout_overlap %.12g" % (k, r, run["overlap"][k, r], float(vol)))
            assert err <= 1e-12 * abs(float(vol))


def test_rooms_do_not_depend_on_the_batch_and_capture_equals_eager():
    both = _run(overlap_weight=WEIGHT)
    for r in (0, 1):
        one = _run(sel=(r,), overlap_weight=WEIGHT)
        _same_bits(one, both, "R = 1 (room %d) against R = 2" % r, (0,), (r,))
        assert np.array_equal(one["overlap"][:, 0], both["overlap"][:, r])
    graph = _run(capture=True, overlap_weight=WEIGHT)
    _same_bits(graph, both, "capture against eager")
    assert np.array_equal(graph["overlap"], both["overlap"])


def test_overlap_rows_exempt_a_room():
    """room 0 with no colliding row: its penalty is 0 and its numbers are those of the loop without the penalty (the head in launches of its
    own computes the same bits); room 1 keeps the default rows"""
    _, _, rooms, _ = _setup()
    n0 = int(rooms[0]["objs"].shape[0])
    part, on, off = _run(overlap_weight=WEIGHT, overlap_rows=((False,) * n0, None)), _run(overlap_weight=WEIGHT), _run()
    assert not part["overlap"][:, 0].any() and np.array_equal(part["overlap"][:, 1], on["overlap"][:, 1])
    _same_bits(part, off, "room 0 exempted", (0,), (0,))
    _same_bits(part, on, "room 1 default", (1,), (1,))


def test_against_the_one_room_loops():
    R, M = pkg("host.refine"), pkg("host.Sg2ScVAE_model")
    _, sd, rooms, bank = _setup()
    batch = _run(overlap_weight=WEIGHT)
    with torch.cuda.stream(torch.cuda.Stream()):
        for r, rm in enumerate(rooms):
            args = (rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"])
            m1 = M.Sg2ScVAEModel(**CFG.model_kwargs()); m1.load_state_dict(sd); m1 = m1.cuda().eval()
            l1, (b1, i1) = R.finetune_vae_fast(m1, *args, iters=ITERS, bank=bank, learning_rate=1e-3, image_size=IMAGE, fused_head=False,
                                               overlap_weight=WEIGHT)
            assert_close(batch["losses"][:, r], l1.cpu().numpy(), "losses of room %d vs finetune_vae_fast" % r, rtol=1e-5)
            assert_close(batch["boxes"][r], b1.cpu().numpy(), "boxes of room %d" % r, rtol=1e-5, atol=1e-6)
            assert_close(batch["idx"][r], i1.cpu().numpy(), "angles of room %d" % r, rtol=1e-5, atol=1e-5)
            assert_close(batch["params"][r], m1.flat_params.detach().cpu().numpy(), "parameters of room %d" % r, rtol=1e-5, atol=1e-7)
            m2 = M.Sg2ScVAEModel(**CFG.model_kwargs()); m2.load_state_dict(sd); m2 = m2.cuda().eval()
            l2, (b2, i2) = R.finetune_vae(m2, *args, iters=ITERS, bank=bank, learning_rate=1e-3, image_size=IMAGE, overlap_weight=WEIGHT)
            assert_close(batch["losses"][:, r], np.asarray(l2), "losses of room %d vs finetune_vae" % r, rtol=2e-3)
            assert_close(batch["boxes"][r], b2.cpu().numpy(), "boxes of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-4)
            assert_close(batch["params"][r], m2.flat_params.detach().cpu().numpy(), "parameters of room %d vs finetune_vae" % r, rtol=1e-3, atol=1e-5)
    torch.cuda.synchronize()


def test_refusals():
    R, EV = pkg("host.refine"), pkg("host.evaluate")
    model, _, rooms, bank = _setup()
    kw = dict(bank=bank, image_size=IMAGE, iters=ITERS)
    for w in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="overlap_weight"):
            R.RefineBatch(model, rooms, overlap_weight=w, **kw)
    unnamed = [dict(rooms[0], class_names=rooms[0]["class_names"][:-1]), rooms[1]]
    with pytest.raises(ValueError, match="class_names"):
        R.RefineBatch(model, unnamed, overlap_weight=1.0, **kw)
    with pytest.raises(ValueError, match="overlap_rows"):
        R.RefineBatch(model, rooms, overlap_weight=1.0, overlap_rows=[[True]], **kw)
    with pytest.raises(ValueError, match="overlap_rows"):
        R.RefineBatch(model, rooms, overlap_weight=1.0, overlap_rows=[[True, False], None], **kw)
    n = EV.MAX_ROOM_ROWS + 1
    big = dict(rooms[0], objs=torch.zeros(n, dtype=torch.int64, device="cuda"), class_names=["bed"] * (n - 1) + ["__room__"])
    with pytest.raises(ValueError, match="more than"):
        R.RefineBatch(model, [big], overlap_weight=1.0, **kw)
    rm = rooms[0]
    with pytest.raises(ValueError, match="overlap_weight"):
        R.finetune_vae_fast(model, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=1, bank=bank,
                            image_size=IMAGE, overlap_weight=-0.5)
    with pytest.raises(ValueError, match="overlap_rows"):
        R.finetune_vae(model, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=1, bank=bank,
                       image_size=IMAGE, overlap_weight=0.5, overlap_rows=[True])
