"""The refinement loop with retrieved meshes (host/refine.py: RefineBatch(retrieve=True), finetune_vae, mesh_render_func): the target shows
the models retrieved for the ground-truth boxes (testing/test_render_refine.py:319), the iterates those retrieved for the first iterate's
boxes (:324-326), frozen from then on.  Small rooms, 64 x 64 images, 3 iterations."""
import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close
from test_mesh_retrieve_host import many_model_bank
from test_refine_gpu import FURN, _random_rooms, _room_model

pytestmark = pytest.mark.gpu

from oracle import vae_ref     # noqa: E402

CFG = dict(embedding_dim=32, gconv_num_layers=2, mlp_normalization="none", decoder_cat=False)
KW = dict(learning_rate=1e-3, image_size=64, iters=3)


def _rooms(n, cfg, seed):
    """rooms whose ground-truth boxes alternate between tall-and-thin (y/x about 4: model 2 of many_model_bank) and flat (y/x about 0.1:
    model 0), while the decoder of _room_model starts every object near (0.3, 0.35, 0.3) of the room - y/x about 0.8, z/x about 1.25:
    model 1.  The retrieval of the targets and that of the iterates therefore differ."""
    rooms = _random_rooms(n, cfg, seed=seed)
    for rm in rooms:
        b = rm["boxes"].clone()
        k = b.shape[0] - 1
        even = torch.arange(k, device=b.device) % 2 == 0
        b[:k, 3] = torch.where(even, b[:k, 0] + 0.1, b[:k, 0] + 0.3)
        b[:k, 4] = torch.where(even, b[:k, 1] + 0.6, b[:k, 1] + 0.05)
        rm["boxes"] = b
    return rooms


def _run(R, model, rooms, bank, **kw):
    rb = R.RefineBatch(model, rooms, bank=bank, **dict(KW, **kw))
    info = rb.launches()
    losses = rb.run().cpu().numpy().copy()
    out = dict(losses=losses, boxes=[b.cpu().numpy().copy() for b, _ in rb.results()], idx=[i.cpu().numpy().copy() for _, i in rb.results()],
               info=info, models=None if rb.models is None else rb.models.cpu().numpy().copy(),
               target_models=None if rb.target_models is None else rb.target_models.cpu().numpy().copy(), F2=rb.F2)
    rb.close()
    return out


def test_one_model_per_class_retrieve_changes_nothing():
    R = pkg("host.refine")
    L = pkg("_lib").lib()
    cfg = vae_ref.VaeConfig(**CFG)
    model, _ = _room_model(cfg)
    rooms = _rooms(3, cfg, seed=5)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    try:
        L.sln_set_deterministic(1)
        with torch.cuda.stream(torch.cuda.Stream()):
            off = _run(R, model, rooms, bank)
            on = _run(R, model, rooms, bank, retrieve=True)
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    assert off["models"] is None and off["target_models"] is None
    is_room = np.concatenate([[False] * (len(rm["class_names"]) - 1) + [True] for rm in rooms])
    assert (on["models"][~is_room] == 0).all() and (on["models"][is_room] == -1).all() and np.array_equal(on["models"], on["target_models"])
    assert np.array_equal(on["losses"], off["losses"]) and on["info"] == off["info"] and on["F2"] == off["F2"]
    assert all(np.array_equal(a, b) for a, b in zip(on["boxes"], off["boxes"])) and all(np.array_equal(a, b) for a, b in zip(on["idx"], off["idx"]))
    assert len(set(on["losses"][:, 0].tolist())) > 1


def test_targets_take_the_ground_truth_retrieval_and_iterates_the_first_iterates():
    R = pkg("host.refine"); RT = pkg("host.retrieve")
    L = pkg("_lib").lib()
    cfg = vae_ref.VaeConfig(**CFG)
    model, _ = _room_model(cfg)
    rooms = _rooms(2, cfg, seed=7)
    bank = many_model_bank(R, FURN, "cuda")
    try:
        L.sln_set_deterministic(1)
        with torch.cuda.stream(torch.cuda.Stream()):
            rb = R.RefineBatch(model, rooms, bank=bank, retrieve=True, **KW)
            assert rb.models is None and rb.target_models is not None
            F2_target = rb.F2
            rb.run(1)                                                        # iteration 0: rb.boxes are the first iterate's
            first = rb.boxes.cpu().clone()
            models, target_models, F2 = rb.models.cpu().clone(), rb.target_models.cpu().clone(), rb.F2
            ids, target_ids = rb.model_ids(), rb.model_ids(target=True)
            losses = rb.run().cpu().numpy().copy()                           # the choice is frozen
            assert torch.equal(rb.models.cpu(), models)
            scene_models = [sc.models for sc in rb.scenes]
            rb.close()
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    table = many_model_bank(R, FURN, "cpu").table
    names = [n for rm in rooms for n in rm["class_names"]]
    cls = torch.tensor([table.vocab.index(n) for n in names], dtype=torch.int32)
    rows = [len(rm["class_names"]) for rm in rooms]
    room_row = torch.from_numpy(np.repeat(np.cumsum(rows) - 1, rows).astype(np.int32))
    gt = torch.cat([rm["boxes"].cpu().float() for rm in rooms])
    assert torch.equal(target_models, RT.retrieve_models_torch(gt, cls, room_row, table))
    assert torch.equal(models, RT.retrieve_models_torch(first, cls, room_row, table))
    obj = room_row != torch.arange(len(room_row))
    assert bool((models[~obj] == -1).all()) and bool((models[obj] >= 0).all())
    differ = obj & (models != target_models)
    # not vacuous: a row whose two choices differ from each other and from model 0
    assert int((differ & (models != 0) & (target_models != 0)).sum()) >= 1, (models.tolist(), target_models.tolist())
    at = 0
    for r, n in enumerate(rows):
        assert list(scene_models[r]) == [max(k, 0) for k in models[at:at + n - 1].tolist()]
        assert ids[r] == [("%s_%d" % (nm, k) if k >= 0 else None) for nm, k in zip(rooms[r]["class_names"], models[at:at + n].tolist())]
        assert target_ids[r] == [("%s_%d" % (nm, k) if k >= 0 else None) for nm, k in zip(rooms[r]["class_names"], target_models[at:at + n].tolist())]
        at += n
    assert F2 != F2_target, "the iterates' meshes have other face counts than the targets': the face buffers were rebound"
    assert np.isfinite(losses).all() and len(set(losses[:, 0].tolist())) > 1


def test_rooms_of_a_batch_equal_the_rooms_alone():
    R = pkg("host.refine")
    L = pkg("_lib").lib()
    cfg = vae_ref.VaeConfig(**CFG)
    model, _ = _room_model(cfg)
    rooms = _rooms(3, cfg, seed=11)
    bank = many_model_bank(R, FURN, "cuda")
    try:
        L.sln_set_deterministic(1)
        with torch.cuda.stream(torch.cuda.Stream()):
            full = _run(R, model, rooms, bank, retrieve=True)
            alone = [_run(R, model, [rm], bank, retrieve=True) for rm in rooms]
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    at = 0
    for r, one in enumerate(alone):
        n = len(rooms[r]["class_names"])
        assert np.array_equal(one["losses"][:, 0], full["losses"][:, r]), "losses of room %d" % r
        assert np.array_equal(one["boxes"][0], full["boxes"][r]) and np.array_equal(one["idx"][0], full["idx"][r]), "layout of room %d" % r
        assert np.array_equal(one["models"], full["models"][at:at + n]) and np.array_equal(one["target_models"], full["target_models"][at:at + n])
        at += n
    assert (full["models"] != full["target_models"]).any() and np.isfinite(full["losses"]).all()


def test_batch_with_retrieval_matches_the_autograd_loop():
    """RefineBatch(retrieve=True) against finetune_vae, whose scenes come from assemble_scene(models=...) per iteration.  Bounds: those of
    tests/test_refine_gpu.py for the fused loop against finetune_vae (losses rtol 2e-3; boxes rtol 1e-3, atol 1e-4)."""
    R = pkg("host.refine"); M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(**CFG)
    model, sd = _room_model(cfg)
    rm = _rooms(1, cfg, seed=7)[0]
    bank = many_model_bank(R, FURN, "cuda")
    with torch.cuda.stream(torch.cuda.Stream()):
        fast = _run(R, model, [rm], bank, retrieve=True)
    torch.cuda.synchronize()
    assert (fast["models"] != fast["target_models"]).any()
    slow_model = M.Sg2ScVAEModel(**cfg.model_kwargs()); slow_model.load_state_dict(sd); slow_model = slow_model.cuda().eval()
    losses, (bp, idx) = R.finetune_vae(slow_model, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"],
                                       bank=bank, **KW)
    print("losses: batch %s, autograd loop %s; max |d boxes| %.3g" % (fast["losses"][:, 0].tolist(), losses,
                                                                        float(np.abs(fast["boxes"][0] - bp.cpu().numpy()).max())))
    assert_close(fast["losses"][:, 0], np.asarray(losses), "losses", rtol=2e-3)
    assert_close(fast["boxes"][0], bp.cpu().numpy(), "boxes", rtol=1e-3, atol=1e-4)


def test_one_room_fused_loop_retrieves_like_the_batch():
    """finetune_vae_fast (target scene from the ground truth's retrieval, iterate scene from iteration 0's) against RefineBatch(retrieve=True)
    on the same room, within the bounds tests/test_refine_gpu.py holds that pair to (losses rtol 1e-5; boxes rtol 1e-5, atol 1e-6)."""
    R = pkg("host.refine"); M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(**CFG)
    model, sd = _room_model(cfg)
    rm = _rooms(1, cfg, seed=7)[0]
    bank = many_model_bank(R, FURN, "cuda")
    with torch.cuda.stream(torch.cuda.Stream()):
        batch = _run(R, model, [rm], bank, retrieve=True)
        m1 = M.Sg2ScVAEModel(**cfg.model_kwargs()); m1.load_state_dict(sd); m1 = m1.cuda().eval()
        l1, (b1, i1) = R.finetune_vae_fast(m1, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], bank=bank, **KW)
        l1, b1 = l1.cpu().numpy(), b1.cpu().numpy()
    torch.cuda.synchronize()
    assert (batch["models"] != batch["target_models"]).any()
    assert_close(batch["losses"][:, 0], l1, "losses", rtol=1e-5)
    assert_close(batch["boxes"][0], b1, "boxes", rtol=1e-5, atol=1e-6)


def test_mesh_render_func_retrieves_once_and_keeps_the_meshes(monkeypatch):
    R = pkg("host.refine"); RT = pkg("host.retrieve"); DR = pkg("host.diff_render")
    names = ["bed", "chair", "sofa", "door", "desk", "__room__"]
    vocab = ["__room__"] + FURN + ["door"]
    objs = [vocab.index(n) for n in names]
    bank = many_model_bank(R, FURN, "cuda")
    R.configure_meshes(vocab, bank)
    boxes = torch.tensor([[0.1, 0.0, 0.1, 0.2, 0.5, 0.18], [0.5, 0.0, 0.2, 0.8, 0.1, 0.5], [0.2, 0.0, 0.6, 0.5, 0.2, 0.9], [0.0, 0.0, 0.3, 0.05, 0.8, 0.6],
                          [0.55, 0.0, 0.6, 0.85, 0.3, 0.9], [0, 0, 0, 4.0, 2.7, 5.0]], device="cuda")
    angles = torch.tensor([0.0, 3.0, 6.0, 0.0, 9.0, 0.0], device="cuda")
    seen = []
    render = DR.scene_render
    monkeypatch.setattr(DR, "scene_render", lambda v, f, *a, **k: (seen.append(int(f.shape[1])), render(v, f, *a, **k))[1])
    final, ids, sizes, _ = R.mesh_render_func([b for b in boxes], [a for a in angles], objs)
    table = bank.table
    cls = torch.tensor([table.vocab.index(n) if n in table.vocab else -1 for n in names], dtype=torch.int32)
    want = RT.retrieve_models_torch(boxes.cpu(), cls, torch.full((6,), 5), many_model_bank(R, FURN, "cpu").table).tolist()
    assert want == [2, 0, 1, -1, 1, -1]
    assert [ids[i] for i in range(5)] == ["bed_2", "chair_0", "sofa_1", "door#0", "desk_1"] and "wall" in ids and final.shape == (1, 70, 256, 256)
    n_shell = sum(f.shape[0] for _, _, f in R.shell_topology(bank))
    faces = lambda ch: n_shell + sum(bank.model_list(n)[k]["f"].shape[0] for n, k in zip(names, ch) if k >= 0)      # noqa: E731
    assert seen == [faces(want)]
    # every box turned flat: a fresh retrieval would take model 0 everywhere - the second call keeps the first call's meshes
    flat = boxes.clone(); flat[:5, 4] = flat[:5, 1] + 0.02; flat[:5, 3] = flat[:5, 0] + 0.3
    again = RT.retrieve_models_torch(flat.cpu(), cls, torch.full((6,), 5), many_model_bank(R, FURN, "cpu").table).tolist()
    assert again == [0, 0, 0, -1, 0, -1] and faces(again) != faces(want)
    _, ids2, sizes2, _ = R.mesh_render_func([b for b in flat], [a for a in angles], objs, model_ids_old=ids, obj_size_target=sizes)
    assert ids2 == {} and seen == [faces(want), faces(want)]
    _, ids3, _, _ = R.mesh_render_func([b for b in flat], [a for a in angles], objs)
    assert [ids3[i] for i in range(5)] == ["bed_0", "chair_0", "sofa_0", "door#0", "desk_0"] and seen[-1] == faces(again)
