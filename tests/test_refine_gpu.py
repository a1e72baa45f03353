"""Layout-refinement path on the GPU (rows B2, B7 and 'next' row f1 of SURVEY.md §8): the placement algebra and the
refinement loss are the same torch code on both sides; the renderer underneath is the fused HIP pass on the GPU and the
33-pass CPU restatement (oracle/raster_ref.py) in the check."""
import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

pytestmark = pytest.mark.gpu

from oracle import raster_ref as rr, refine_ref, vae_ref     # noqa: E402

NAMES = ["bed", "chair", "table", "sofa", "door", "desk", "__room__"]       # 'door' is skipped by the reference (DO_NOT_VIS)


def _inputs(dev):
    g = torch.Generator().manual_seed(0)
    lo = torch.rand(len(NAMES), 3, generator=g) * 0.45 + 0.05
    lo[:, 1] = 0.0; lo[:, 2] = lo[:, 2] * 0.6
    hi = lo + torch.rand(len(NAMES), 3, generator=g) * 0.2 + 0.12
    boxes = torch.cat([lo, hi], 1)
    boxes[-1] = torch.tensor([0, 0, 0, 4.0, 2.7, 5.0])
    angles = torch.randint(0, 24, (len(NAMES),), generator=g).float()
    return boxes.to(dev), angles.to(dev)


def test_scene_assembly_and_refinement_loss_match_cpu_restatement():
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    res = {}
    for dev, render in (("cpu", rr.scene_render), ("cuda", DR.scene_render)):
        boxes, angles = _inputs(dev)
        bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], dev, seed=3)
        room = boxes[-1].clone()
        v0, f0, ranges, sizes, _ = R.assemble_scene(boxes, angles, NAMES, bank, room)
        with torch.no_grad():
            target = render(v0, f0, ranges, room, image_size=96)
        labels = R.target_labels(target)
        b2 = (boxes + 0.02).detach().requires_grad_(True)
        a2 = (angles + 0.7).detach().requires_grad_(True)
        v, f, ranges, _, size_loss = R.assemble_scene(b2, a2, NAMES, bank, room, [s.clone() for s in sizes])
        img = render(v, f, ranges, room, image_size=96)
        loss, dl, sl = R.refinement_loss(img, target, labels, size_loss)
        loss.backward()
        res[dev] = (loss.item(), dl.item(), sl.item(), b2.grad.cpu().numpy(), a2.grad.cpu().numpy(), target.cpu().numpy())
    c, g = res["cpu"], res["cuda"]
    # a few silhouette pixels may land on the other side (torch's CPU and GPU matmuls round the projection differently): counted.
    # Bounds as the reference-executed fixtures justify them (tests/test_refine_golden_gpu.py: loss / boxes / angles 1e-4 over four
    # iterations of the whole loop; gradients THROUGH silhouettes 5e-3 of their largest entry)
    flipped = int((np.abs(c[5] - g[5]) > 1e-4).any(1).sum())
    assert flipped <= 8, "%d of %d pixels differ" % (flipped, c[5].shape[-1] ** 2)
    assert abs(c[0] - g[0]) <= 2e-4 * abs(c[0]), (c[0], g[0])
    assert abs(c[1] - g[1]) <= 5e-4 * abs(c[1]) and abs(c[2] - g[2]) <= 1e-4 * abs(c[2]), (c[1], g[1], c[2], g[2])
    assert_close(g[3], c[3], "d loss / d boxes", rtol=5e-3, atol=0)
    assert_close(g[4], c[4], "d loss / d angles", rtol=5e-3, atol=0)
    assert np.abs(c[3]).max() > 0 and np.abs(c[4]).max() > 0


def test_finetune_loop_runs_on_device_and_reduces_the_loss():
    """decoder -> softargmax -> placement -> fused render -> PSP losses -> SGD on z, 10 iterations on the device.
    The tiny VAE is first over-fitted to the room (a random decoder puts every object outside the view)."""
    R = pkg("host.refine"); M = pkg("host.Sg2ScVAE_model")
    torch.manual_seed(0)                     # the model seeds its on-device eps draws from torch.initial_seed(): do not depend on the tests run before
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="none")
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict(vae_ref.init_state(cfg, seed=1))
    model = model.cuda().train()
    boxes, angles = _inputs("cuda")
    n = len(NAMES)
    objs = torch.tensor([3, 4, 6, 5, 7, 13, 0], device="cuda")
    triples = torch.tensor([[0, 1, 1], [2, 3, 3], [1, 2, 5]] + [[i, 0, n - 1] for i in range(n - 1)], device="cuda")
    attrs = torch.zeros(n, dtype=torch.int64, device="cuda")
    nb = boxes.clone(); nb[-1] = torch.tensor([0, 0, 0, 1.0, 1.0, 1.0], device="cuda")      # dataset boxes are room-normalised
    for _ in range(400):
        model.train_step(objs, triples, nb, angles.long(), attrs, kl_weight=1e-3, lr=2e-3, use_graph=False)
    # (400 Adam steps with atomically accumulated gradients end in a slightly different model every run; twenty refinement
    # iterations lower the loss from every one of them, ten did not always - six repeated runs, tools notes in DESIGN.md)
    losses, (bp, idx) = R.finetune_vae(model, objs, triples, boxes, angles.long(), attrs, NAMES, iters=20, image_size=96,
                                        learning_rate=1e-3)
    assert len(losses) == 20 and all(np.isfinite(losses))
    assert torch.isfinite(bp).all() and torch.isfinite(idx).all()
    assert len(set(losses)) > 1, "no gradient reached z"
    assert min(losses[1:]) < losses[0]


def test_mesh_render_func_call_contract():
    """models/diff_render.py:48,435: list inputs, 4-tuple output, first call caches ids / sizes / room box, later calls
    reuse them and return the size + wall-drift penalty; the image equals assemble_scene + scene_render."""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    boxes, angles = _inputs("cuda")
    vocab = ["__pad__"] + NAMES
    objs = [vocab.index(n) for n in NAMES]
    bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], "cuda", seed=3)
    R.configure_meshes(vocab, bank)
    final, ids, sizes, size_loss = DR.mesh_render_func([b for b in boxes], [a for a in angles], objs)
    assert final.shape == (1, 70, 256, 256) and float(size_loss) == 0.0
    n_vis = sum(1 for n in NAMES[:-1] if n not in R.DO_NOT_VIS)
    assert len(sizes) == n_vis + 1 and np.allclose(ids["box_info"], boxes[-1].cpu().numpy())
    assert all(i in ids for i in range(len(NAMES) - 1)) and "wall" in ids
    v, f, ranges, _, _ = R.assemble_scene(boxes, angles, NAMES, bank, boxes[-1])
    assert torch.equal(final, DR.scene_render(v, f, ranges, boxes[-1]))
    # second call: perturbed layout, drifting room row is overloaded by the cached one and penalised
    b2 = [(b + 0.01).detach().requires_grad_(True) for b in boxes]
    a2 = [a.detach().clone().requires_grad_(True) for a in angles]
    final2, ids2, sizes2, loss2 = DR.mesh_render_func(b2, a2, objs, model_ids_old=ids, obj_size_target=sizes)
    assert ids2 == {} and sizes2 == []
    room = boxes[-1]
    want = sum(torch.nn.functional.mse_loss(((boxes[i] + 0.01)[3:] - (boxes[i] + 0.01)[:3]) * room[3:],
                                            torch.from_numpy(sizes[k]).cuda())
               for k, i in enumerate(j for j, n in enumerate(NAMES[:-1]) if n not in R.DO_NOT_VIS))
    want = want + torch.nn.functional.mse_loss(boxes[-1] + 0.01, boxes[-1])
    assert abs(float(loss2.detach()) - float(want)) <= 1e-6 + 1e-5 * float(want)
    (final2[:, 41:].sum() + loss2).backward()
    assert all(b.grad is not None and torch.isfinite(b.grad).all() for b in b2[:-1])
    assert any(float(b.grad.abs().max()) > 0 for b in b2[:-1])


def test_caller_supplied_meshes_render_through_mesh_render_func():
    """MeshBank.from_arrays: non-cuboid meshes handed in as (V, F) arrays (the reference retrieves SUNCG models at
    models/diff_render.py:62,131) go through mesh_render_func, the fused placement (RefineScene) and the CPU restatement with the
    same image and gradients."""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    octa_v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1.3, 0], [0, -0.7, 0], [0, 0, 0.8], [0, 0, -0.8]], np.float32) * 0.4
    octa_f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    wedge_v = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0.6], [0, 0, 0.6], [0, 0.9, 0], [0, 0.9, 0.6]], np.float32)
    wedge_f = np.array([[0, 1, 2], [0, 2, 3], [0, 4, 1], [3, 2, 5], [0, 3, 5], [0, 5, 4], [1, 4, 5], [1, 5, 2]])
    meshes = {"bed": (octa_v, octa_f), "chair": (wedge_v, wedge_f), "table": (octa_v * 1.5 + 0.1, octa_f[:, ::-1]), "sofa": (wedge_v, wedge_f),
              "desk": (octa_v, octa_f)}
    with pytest.raises(IndexError):
        R.MeshBank.from_arrays({"bed": (octa_v, octa_f + 3)}, "cuda")
    res = {}
    for dev, render in (("cpu", rr.scene_render), ("cuda", DR.scene_render)):
        boxes, angles = _inputs(dev)
        bank = R.MeshBank.from_arrays(meshes, dev)
        assert bank.models["bed"]["v"].shape == (6, 3) and torch.allclose(bank.models["chair"]["bbox_max"].cpu(), torch.tensor([1.0, 0.9, 0.6]))
        room = boxes[-1].clone()
        b2 = boxes.detach().clone().requires_grad_(True); a2 = (angles + 0.3).detach().requires_grad_(True)
        v, f, ranges, sizes, _ = R.assemble_scene(b2, a2, NAMES, bank, room)
        img = render(v, f, ranges, room, image_size=96)
        (img[:, 41:].sum() + img[:, 0].mean()).backward()
        res[dev] = (img.detach().cpu().numpy(), b2.grad.cpu().numpy(), a2.grad.cpu().numpy(), bank)
    assert (np.abs(res["cpu"][0] - res["cuda"][0]) > 1e-4).mean() < 1e-3
    assert_close(res["cuda"][1], res["cpu"][1], "d boxes", rtol=2e-2, atol=2e-2 * np.abs(res["cpu"][1]).max())
    assert_close(res["cuda"][2], res["cpu"][2], "d angles", rtol=2e-2, atol=2e-2 * np.abs(res["cpu"][2]).max())
    assert np.abs(res["cpu"][1]).max() > 0
    # the reference's entry point on the same bank, and the fused placement against the per-object assembly
    bank = res["cuda"][3]
    boxes, angles = _inputs("cuda")
    R.configure_meshes(NAMES, bank=bank)
    final, ids, sizes, size_loss = R.mesh_render_func([b for b in boxes], [a for a in angles], list(range(len(NAMES))))
    assert final.shape == (1, 70, 256, 256) and float(final[0, 0].max()) > 0
    sc = R.RefineScene(NAMES, bank, boxes[-1], 96)
    with torch.no_grad():
        fused, _, _ = sc.render(boxes, angles)
        v, f, ranges, _, _ = R.assemble_scene(boxes, angles, NAMES, bank, boxes[-1])
        plain = DR.scene_render(v, f, ranges, boxes[-1], image_size=96)
    assert (np.abs(fused.cpu().numpy() - plain.cpu().numpy()) > 1e-4).mean() < 1e-3


def _pretrained_room():
    M = pkg("host.Sg2ScVAE_model")
    torch.manual_seed(0)                                            # train_step draws eps from the global device generator
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="none")
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict(vae_ref.init_state(cfg, seed=1))
    model = model.cuda().train()
    boxes, angles = _inputs("cuda")
    n = len(NAMES)
    objs = torch.tensor([3, 4, 6, 5, 7, 13, 0], device="cuda")
    triples = torch.tensor([[0, 1, 1], [2, 3, 3], [1, 2, 5]] + [[i, 0, n - 1] for i in range(n - 1)], device="cuda")
    attrs = torch.zeros(n, dtype=torch.int64, device="cuda")
    nb = boxes.clone(); nb[-1] = torch.tensor([0, 0, 0, 1.0, 1.0, 1.0], device="cuda")
    for _ in range(400):
        model.train_step(objs, triples, nb, angles.long(), attrs, kl_weight=1e-3, lr=2e-3, use_graph=False)
    return model, objs, triples, boxes, angles, attrs


@pytest.mark.parametrize("fused", [True, False])
def test_batched_scene_equals_per_object_assembly(fused):
    """RefineScene (fused: csrc/placement.hip - placement, projection, cull, fill_back, size loss in one kernel each way;
    otherwise the batched torch expression) against the per-object assembly of diff_render.py:76-165."""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    boxes, angles = _inputs("cuda")
    bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], "cuda", seed=3)
    room = boxes[-1].clone()
    tgt = [torch.tensor([0.5, 0.4, 0.6], device="cuda") * (1 + 0.1 * k) for k in range(5)]
    b1 = boxes.clone().requires_grad_(True); a1 = (angles + 0.3).clone().requires_grad_(True)
    v, f, ranges, sizes, sl1 = R.assemble_scene(b1, a1, NAMES, bank, room, tgt)
    img1 = DR.scene_render(v, f, ranges, room, image_size=128)
    scene = R.RefineScene(NAMES, bank, room, image_size=128)
    assert scene.n_vis == len(tgt)
    b2 = boxes.clone().requires_grad_(True); a2 = (angles + 0.3).clone().requires_grad_(True)
    img2, sl2, size2 = scene.render(b2, a2, torch.stack(tgt), fused=fused)
    assert torch.equal(torch.stack(sizes), size2.detach())
    assert abs(float(sl1.detach()) - float(sl2.detach())) <= 1e-6 * abs(float(sl1.detach())) and float(sl1.detach()) > 0
    assert ((img1 - img2).abs() > 1e-4).float().mean() < 1e-3   # batched vs per-object matmul rounding: a few silhouette pixels
    w = torch.randn(img1.shape, generator=torch.Generator().manual_seed(0)).cuda()
    ((img1 * w).sum() + 3.0 * sl1).backward(); ((img2 * w).sum() + 3.0 * sl2).backward()
    assert_close(b2.grad.cpu().numpy(), b1.grad.cpu().numpy(), "d/d boxes", rtol=2e-3, atol=2e-3 * float(b1.grad.abs().max()))
    assert_close(a2.grad.cpu().numpy(), a1.grad.cpu().numpy(), "d/d angles", rtol=2e-3, atol=2e-3 * float(a1.grad.abs().max()))
    assert float(b1.grad[4].abs().max()) == 0.0 and float(b2.grad[4].abs().max()) == 0.0      # 'door' is not placed
    # the size loss alone (no image term): exact chain rule, tight tolerance
    b3 = boxes.clone().requires_grad_(True)
    _, sl3, _ = scene.render(b3, angles + 0.3, torch.stack(tgt), fused=fused)
    sl3.backward()
    b4 = boxes.clone().requires_grad_(True)
    R.assemble_scene(b4, angles + 0.3, NAMES, bank, room, tgt)[4].backward()
    assert_close(b3.grad.cpu().numpy(), b4.grad.cpu().numpy(), "d size_loss / d boxes", rtol=1e-5)


def test_fast_finetune_loop_matches_the_reference_shaped_loop_and_its_graph_replay():
    R = pkg("host.refine")
    bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], "cuda", seed=3)
    runs = {}
    model0, objs, triples, boxes, angles, attrs = _pretrained_room()
    sd0 = {k: v.detach().clone() for k, v in model0.state_dict().items()}     # fp32 atomics make two trainings differ in the last bits
    M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="none")
    for mode in ("slow", "fast", "graph"):
        model = M.Sg2ScVAEModel(**cfg.model_kwargs()); model.load_state_dict(sd0); model = model.cuda().train()
        if mode == "slow":
            losses, (bp, idx) = R.finetune_vae(model, objs, triples, boxes, angles.long(), attrs, NAMES, iters=6, image_size=96,
                                               learning_rate=1e-3, bank=bank)
        else:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                losses, (bp, idx) = R.finetune_vae_fast(model, objs, triples, boxes, angles.long(), attrs, NAMES, iters=6, image_size=96,
                                                        learning_rate=1e-3, bank=bank, capture=(mode == "graph"))
                losses = losses.tolist()
            torch.cuda.synchronize()
        runs[mode] = (np.asarray(losses), bp.cpu().numpy(), model.flat_params.detach().cpu().numpy().copy())
    for mode in ("fast", "graph"):
        assert_close(runs[mode][0], runs["slow"][0], mode + ": losses", rtol=2e-3)
        assert_close(runs[mode][1], runs["slow"][1], mode + ": boxes", rtol=1e-3, atol=1e-4)
        assert_close(runs[mode][2], runs["slow"][2], mode + ": parameters", rtol=1e-3, atol=1e-5)
    assert len(set(runs["graph"][0].tolist())) > 1


def _target_and_iterate(image_size, batch):
    """Two renders of the same room, the second with its objects moved and turned: (target, iterate) of the loss tests"""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    boxes, angles = _inputs("cuda")
    bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], "cuda", seed=3)
    room = boxes[-1].clone()
    v0, f0, ranges, sizes, _ = R.assemble_scene(boxes, angles, NAMES, bank, room)
    with torch.no_grad():
        target = DR.scene_render(v0, f0, ranges, room, image_size=image_size)
        b2 = boxes + 0.03; b2[-1] = boxes[-1]
        v, f, ranges, _, _ = R.assemble_scene(b2, angles + 0.7, NAMES, bank, room)
        img = DR.scene_render(v, f, ranges, room, image_size=image_size)
        if batch == 2:                                            # second sample: the roles swapped (cross_entropy / l1 average over the batch)
            target, img = torch.cat([target, img]), torch.cat([img, target])
    return target, img


def _torch_loss_and_gradient(rl, target, img):
    """The oracle of the loss tests - the reference's torch calls on the CPU, in fp64 and in fp32: {dtype: ([loss, depth, sem], gradient)}"""
    # labels: the product derives them from its own resampling of the target; torch's resampling must agree on them
    lab_t = torch.cat(refine_ref.target_labels(target.cpu()), 1)
    assert (lab_t != rl.labels.cpu().long()).float().mean() < 2e-3
    labels = [rl.labels[:, k:k + 1].cpu().long() for k in range(rl.labels.shape[1])]
    ref = {}
    for dt in (torch.float64, torch.float32):
        xi = img.cpu().to(dt).requires_grad_(True)
        loss, dl, sl = refine_ref.refinement_loss(xi, target.cpu().to(dt), labels, torch.zeros((), dtype=dt))     # the oracle: the reference's torch calls
        loss.backward()
        ref[dt] = ([float(loss.detach()), float(dl.detach()), float(sl.detach())], xi.grad.numpy())
    return ref


@pytest.mark.parametrize("image_size,batch", [(256, 1), (96, 1), (96, 2)])
def test_fused_refinement_loss_matches_the_torch_ops(image_size, batch):
    """csrc/refine_loss.hip (null-fill, PSP pooling, L1, cross-entropy; backward through the transposed resampling) against
    the reference's own formulation - F.interpolate / l1_loss / cross_entropy (test_render_refine.py:192-215,328-356) -
    evaluated on the CPU in fp64 and fp32 on the same two images."""
    R = pkg("host.refine")
    target, img = _target_and_iterate(image_size, batch)
    rl = R.RefineLoss(target)
    x = img.clone().requires_grad_(True)
    out = rl(x)
    (out[0] * 1.5).backward()                                     # a non-trivial incoming gradient
    got = [float(t) for t in out.detach().cpu()]
    g = x.grad.cpu().numpy() / 1.5
    ref = _torch_loss_and_gradient(rl, target, img)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    for a, b, nm in zip(got, r64[0], ("total", "depth", "semantic")):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (nm, a, b)
    # gradient: the L1 part is sign(diff) * const, so pooled pixels whose |diff| is at rounding level may flip; the fp32
    # evaluation of the reference itself shows how many do
    scale = np.abs(r64[1]).max()
    bad = np.abs(g - r64[1]) > 1e-4 * scale
    bad32 = np.abs(r32[1] - r64[1]) > 1e-4 * scale
    assert scale > 0 and (g[:, 0] == 0).all()
    assert bad.mean() <= max(4.0 * bad32.mean(), 1e-5), (bad.mean(), bad32.mean())
    assert np.abs(g - r64[1]).max() <= 1e-4 * scale + 4.0 * np.abs(r32[1] - r64[1]).max()
    # identical images: the depth part vanishes exactly and its gradient is exactly zero (both go through the same kernel)
    y = target.clone().requires_grad_(True)
    o2 = rl(y)
    o2[0].backward()
    filled = y.grad[:, -1].abs().sum() + y.grad[:, 41:-1].abs().sum()
    null = (target[:, 41:].sum(1) < 0.5)
    assert float(y.grad[:, 41:-1].abs().max()) == 0.0
    assert float(y.grad[:, -1][null].abs().max() if null.any() else 0.0) == 0.0 and torch.isfinite(filled)


def test_fused_refinement_loss_with_plane_flags_and_neither_optional_table():
    """SlnRefineLoss::live_planes WITHOUT null_mask and pooled_ones (the rooms-in-flight loop always hands over all three): the loss
    then computes the null mask itself, through the flags, and pools a plane flagged "the constant 1" from 1.f.  The flags are read off
    the iterate (a plane of zeros: 0, a depth-hot plane of ones: 1, else 3), so the image they describe is the image itself and the
    torch expressions of the test above apply, at its tolerances; planes whose gradient nobody reads keep what the buffer held."""
    import ctypes as C
    R = pkg("host.refine"); _lib = pkg("_lib")
    target, img = _target_and_iterate(96, 2)
    img = img.clone()
    # a window without depth-hot values: null pixels in sample 1; in sample 0 one depth-hot plane is the constant 1 throughout, which
    # alone keeps the window's sums at 1 - not null, but only for a mask that counts the flagged plane
    flat = [c for c in range(41, 69) if float(img[0, c].min()) == float(img[0, c].max())]      # planes of classes the room does not show
    assert flat, "no constant depth-hot plane in sample 0"
    img[:, 41:, 10:40, 20:70] = 0.0
    img[0, flat[0]] = 1.0
    live = torch.full(img.shape[:2], 3, dtype=torch.uint8)
    for b in range(img.shape[0]):
        for c in range(1, 69):
            plane = img[b, c]
            if not bool(plane.any()):
                live[b, c] = 0
            elif c >= 41 and bool((plane == 1.0).all()):
                live[b, c] = 1
    assert (live[:, 1:41] == 0).any() and (live[:, 1:41] == 3).any() and (live[0, 41:] == 1).any() and (live[:, 41:69] == 3).any()
    null = img[:, 41:].sum(1) < 0.5
    assert not bool(null[0].any()) and bool(null[1, 10:40, 20:70].all())
    live_dev = live.cuda()
    rl = R.RefineLoss(target)
    assert _lib.lib().sln_refine_loss_live_ok(C.byref(rl.desc)) == 1
    rl.desc.live_planes = live_dev.data_ptr()
    assert not rl.desc.null_mask and not rl.desc.pooled_ones
    with torch.no_grad():
        out = rl(img)
    got = [float(t) for t in out.cpu()]
    sentinel = 7.0
    g_dev, g_scale = torch.full(img.shape, sentinel, device="cuda"), torch.full((1,), 1.5, device="cuda")
    _lib.check(_lib.lib().sln_refine_loss_backward(rl.desc, _lib.ptr(rl.ws), _lib.ptr(g_scale), _lib.ptr(g_dev),
                                                   _lib.current_stream_ptr()), "sln_refine_loss_backward")
    g = g_dev.cpu().numpy()
    ref = _torch_loss_and_gradient(rl, target, img)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    for a, b, nm in zip(got, r64[0], ("total", "depth", "semantic")):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (nm, a, b)
    read = ((live.numpy() & 2) != 0)                               # [B, C]: planes whose gradient is written
    assert (g[~read] == sentinel).all()
    g, g64, g32 = g[read] / 1.5, r64[1][read], r32[1][read]
    scale = np.abs(r64[1]).max()
    bad = np.abs(g - g64) > 1e-4 * scale
    bad32 = np.abs(g32 - g64) > 1e-4 * scale
    assert scale > 0 and bool((g_dev[:, 0] == 0).all()) and bool((g_dev[1, -1][null[1]] == 0).all())
    assert bad.mean() <= max(4.0 * bad32.mean(), 1e-5), (bad.mean(), bad32.mean())
    assert np.abs(g - g64).max() <= 1e-4 * scale + 4.0 * np.abs(g32 - g64).max()


def test_room_without_visible_objects():
    """Only classes mesh_render_func skips (diff_render.py:93-97): the scene is the room shell, gradients are zero."""
    R = pkg("host.refine")
    names = ["door", "window", "__room__"]
    boxes = torch.tensor([[0.1, 0, 0.1, 0.3, 0.5, 0.2], [0.5, 0.2, 0.0, 0.7, 0.6, 0.05], [0, 0, 0, 4.0, 2.7, 5.0]], device="cuda")
    angles = torch.tensor([3.0, 7.0, 0.0], device="cuda")
    bank = R.MeshBank([], "cuda", seed=0)
    scene = R.RefineScene(names, bank, boxes[-1].clone(), image_size=96)
    assert scene.n_vis == 0
    outs = []
    for fused in (True, False):
        b = boxes.clone().requires_grad_(True); a = angles.clone().requires_grad_(True)
        img, sl, size = scene.render(b, a, None, fused=fused)
        assert size.shape[0] == 0 and float(sl.detach()) == 0.0
        (img.sum() + sl).backward()
        assert float(b.grad.abs().max()) == 0.0 and float(a.grad.abs().max()) == 0.0
        outs.append(img.detach())
    assert torch.equal(outs[0], outs[1]) and float((outs[0][:, 0] > 0).float().mean()) > 0.5       # the shell is visible


def test_fused_placement_matches_the_restated_object_loop():
    """csrc/placement.hip against oracle/refine_ref.py::place_scene (diff_render.py:76-165 statement by statement, 4x4 transforms
    and python min() included) in fp64 on the CPU: placed vertices through the camera, sizes, size loss and the gradients w.r.t.
    the box rows and angle bins of a scalar function of the projected faces."""
    R = pkg("host.refine"); DR = pkg("host.diff_render"); NRm = pkg("host.neural_renderer")
    boxes, angles = _inputs("cuda")
    bank = R.MeshBank([n for n in NAMES if n not in R.DO_NOT_VIS and n != "__room__"], "cuda", seed=3)
    room = boxes[-1].clone()
    scene = R.RefineScene(NAMES, bank, room, image_size=96)
    tgt = torch.stack([torch.tensor([0.5, 0.4, 0.6]) * (1 + 0.1 * k) for k in range(scene.n_vis)])
    b = boxes.clone().requires_grad_(True); a = (angles + 0.3).clone().requires_grad_(True)
    fxyz, sl, size = R._PlaceFn.apply(b, a, scene, tgt.cuda())
    Fn = scene.faces.shape[0]
    w = torch.randn(Fn, 3, 3, generator=torch.Generator().manual_seed(1)).cuda()
    (fxyz[:Fn] * w).sum().add(3.0 * sl).backward()
    # ---- oracle, fp64 on the CPU
    models = {k: {kk: vv.detach().cpu().double() for kk, vv in m.items() if kk != "f"} for k, m in bank.models.items()}
    b64 = boxes.detach().cpu().double().requires_grad_(True); a64 = (angles + 0.3).detach().cpu().double().requires_grad_(True)
    # during the optimisation the room row is the cached constant (diff_render.py:55-57: boxes[-1] = model_ids_old["box_info"])
    b_in = torch.cat([b64[:-1], boxes[-1:].detach().cpu().double()])
    verts, sizes, sl64 = refine_ref.place_scene(b_in, a64, NAMES, models, [t.double() for t in tgt])
    K, Rm, t = [x.cpu().double() for x in (scene.K, scene.R, scene.t)]
    allv = torch.cat([verts, scene.shell_v.cpu().double()])[None]
    # objects occupy Vm vertex slots each in the product's table: map its face list to the compact oracle numbering
    Vm = scene.desc.Vm
    counts = [bank.models[NAMES[i]]["v"].shape[0] for i in scene.vis.tolist()]
    remap = torch.full((scene.n_vis * Vm + scene.shell_v.shape[0],), -1, dtype=torch.int64)
    off = 0
    for k, c in enumerate(counts):
        remap[k * Vm:k * Vm + c] = torch.arange(off, off + c); off += c
    remap[scene.n_vis * Vm:] = torch.arange(off, off + scene.shell_v.shape[0])
    faces = remap[scene.faces.cpu()]
    assert (faces >= 0).all()
    ref = rr.vertices_to_faces(rr.project(allv, K, Rm, t, 512), faces[None])[0]          # [F,3,3]
    cam_z = (torch.matmul(allv, Rm.transpose(1, 2)) + t)[0, :, 2]
    culled = (cam_z[faces] < DR.CULL_EPS).any(1)
    ref = torch.where(culled[:, None, None], torch.zeros_like(ref), ref)
    ((ref * w.cpu().double()).sum() + 3.0 * sl64).backward()
    assert_close(fxyz[:Fn].detach().cpu().numpy(), ref.detach().numpy(), "projected faces", rtol=1e-5, atol=1e-5)
    assert_close(fxyz[Fn:].detach().cpu().numpy(), ref.detach().numpy()[:, [2, 1, 0]], "fill_back copies", rtol=1e-5, atol=1e-5)
    assert_close(size.cpu().numpy(), torch.stack(sizes).detach().numpy(), "sizes", rtol=1e-6)
    assert_close(float(sl.detach()), float(sl64.detach()), "size loss", rtol=1e-5)
    assert_close(b.grad.cpu().numpy(), b64.grad.numpy(), "d/d boxes", rtol=2e-4, atol=2e-4 * float(b64.grad.abs().max()))
    assert float(b.grad[-1].abs().max()) == 0.0
    assert_close(a.grad.cpu().numpy(), a64.grad.numpy(), "d/d angles", rtol=2e-4, atol=2e-4 * float(a64.grad.abs().max()))
    assert float(b64.grad.abs().max()) > 0 and float(a64.grad.abs().max()) > 0


def test_refinement_loss_generic_backward_kernel_and_other_scales():
    """The backward pass has two kernels: the separable one (column lists of at most 5 entries, pooled size <= 96) and a generic
    CSR walk for everything else.  Both must give the same gradient; a different set of scales (and a pooled size of 80) goes
    through the torch formulation as well."""
    R = pkg("host.refine")
    g = torch.Generator().manual_seed(5)
    target = torch.rand(1, 70, 128, 128, generator=g).cuda()
    target[:, 1:41] = (target[:, 1:41] > 0.9).float()
    img = (target + 0.1 * torch.randn(1, 70, 128, 128, generator=g).cuda()).clamp(0, 1)
    for sizes in ((32, 48, 64, 96), (20, 56, 80)):
        rl = R.RefineLoss(target, sizes=sizes)
        x = img.clone().requires_grad_(True)
        out = rl(x); out[0].backward()
        g_fast = x.grad.clone()
        rl.desc.max_col_entries = 0                                  # 'unknown': forces the generic kernel
        x2 = img.clone().requires_grad_(True)
        out2 = rl(x2); out2[0].backward()
        assert torch.equal(out.detach(), out2.detach())
        assert_close(x2.grad.cpu().numpy(), g_fast.cpu().numpy(), "generic vs separable backward %s" % (sizes,), rtol=1e-5,
                     atol=1e-6 * float(g_fast.abs().max()))
        labels = [rl.labels[:, k:k + 1].cpu().long() for k in range(len(sizes))]
        xi = img.cpu().double().requires_grad_(True)
        loss, dl, sl = refine_ref.refinement_loss(xi, target.cpu().double(), labels, torch.zeros((), dtype=torch.float64), sizes=sizes)
        loss.backward()
        assert abs(float(out[0].detach()) - float(loss.detach())) <= 1e-4 * abs(float(loss.detach()))
        scale = float(xi.grad.abs().max())
        bad = (np.abs(g_fast.cpu().numpy() - xi.grad.numpy()) > 1e-4 * scale).mean()
        assert bad < 2e-3, (sizes, bad)                               # L1 sign flips at rounding level only


def test_fused_head_and_update_match_the_torch_expressions():
    """_HeadFn (soft-argmax + noise + the two cats, fix_grad / quad_grad in backward) and sln_refine_sgd against the torch ops
    of finetune_vae (testing/test_render_refine.py:20-25, 217-228, 286-306)."""
    R = pkg("host.refine")
    L = pkg("_lib")
    torch.manual_seed(3)
    n, na = 13, 24
    bp = torch.randn(n, 6, device="cuda", requires_grad=True)
    ap = (torch.randn(n, na, device="cuda") * 3).requires_grad_(True)
    noise = torch.randn(n, device="cuda")
    box_last, angle_last = torch.rand(6, device="cuda"), torch.tensor([7.0], device="cuda")
    wb, wi = torch.randn(n, 6, device="cuda"), torch.randn(n, device="cuda")
    # reference expression
    bp1, ap1 = bp.detach().clone().requires_grad_(True), ap.detach().clone().requires_grad_(True)
    b1 = bp1 * 1.0
    b1.register_hook(R.fix_grad)
    full1 = torch.cat([b1[:-1], box_last[None]], 0)
    i1 = R.softargmax(ap1, sum_dim=1) + noise / 10.0
    i1.register_hook(R.quad_grad)
    i1 = torch.cat([i1[:-1], angle_last], 0)
    ((full1 * wb).sum() + (i1 * wi).sum()).backward()
    full2, i2 = R._HeadFn.apply(bp, ap, noise, box_last, angle_last, 2.0)
    ((full2 * wb).sum() + (i2 * wi).sum()).backward()
    assert_close(full2.detach().cpu().numpy(), full1.detach().cpu().numpy(), "boxes_full", rtol=0, atol=0)
    assert_close(i2.detach().cpu().numpy(), i1.detach().cpu().numpy(), "idx", rtol=1e-5, atol=1e-5)
    assert_close(bp.grad.cpu().numpy(), bp1.grad.cpu().numpy(), "d boxes_pred", rtol=1e-6, atol=1e-7)
    assert_close(ap.grad.cpu().numpy(), ap1.grad.cpu().numpy(), "d angles_pred", rtol=1e-4, atol=1e-6)
    # update: p -= step g, g = 0, z -= step_z gz (sizes that are not multiples of four)
    for npar in (1031, 4096, 3):
        p, g = torch.randn(npar, device="cuda"), torch.randn(npar, device="cuda")
        z, gz = torch.randn(13, 64, device="cuda"), torch.randn(13, 64, device="cuda")
        p0, z0 = p - 0.011 * g, z - 0.00022 * gz
        L.check(L.lib().sln_refine_sgd(L.ptr(p), L.ptr(g), npar, 0.011, L.ptr(z), L.ptr(gz), z.numel(), 0.00022, L.current_stream_ptr()), "sgd")
        assert_close(p.cpu().numpy(), p0.cpu().numpy(), "params", rtol=1e-6, atol=1e-7)
        assert_close(z.cpu().numpy(), z0.cpu().numpy(), "z", rtol=1e-6, atol=1e-7)
        assert float(g.abs().max()) == 0.0


# ----------------------------------------------------------------------------- R rooms in flight (round 5)
def sd_flat(model):
    return model.flat_params.detach().cpu().numpy()


FURN = ["bed", "chair", "table", "sofa", "desk", "cabinet", "lamp", "television", "bookshelf", "dresser", "night_stand", "shelves"]


def _random_rooms(R, cfg, seed=0, dev="cuda"):
    """R rooms of 4 .. 13 objects (+ the room row): boxes inside the room, a relation per object plus the in-room triples"""
    rng = np.random.default_rng(seed)
    rooms = []
    for r in range(R):
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


def _room_model(cfg, seed=1):
    """a decoder that puts the objects INSIDE the view (a random one places them anywhere: no pixel, no gradient)"""
    M = pkg("host.Sg2ScVAE_model")
    sd = vae_ref.init_state(cfg, seed=seed, scale=0.3)
    last = "box_net.%d.bias" % (3 if cfg.mlp_normalization == "batch" else 2)
    sd[last] = torch.tensor([0.25, 0.0, 0.2, 0.55, 0.35, 0.5])
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict(sd)
    return model.cuda().eval(), sd


@pytest.mark.parametrize("which", ["train_py_defaults", "small_no_norm_z_behind_the_gconvs"])
def test_rooms_in_flight_equal_the_one_room_loop(which, monkeypatch):
    """testing/test_render_refine.py:250-263 refines its rooms one after the other, every one on a fresh copy of the checkpoint.
    RefineBatch runs R of them as one launch sequence: a room's losses, boxes, angles, latents and fine-tuned parameters must not
    depend on the other rooms of the batch - BIT-identical between R = 16, R = 3 and R = 1 in deterministic mode, also under
    hipGraph replay - and agree with the autograd-based one-room loop (finetune_vae_fast, other GEMM bodies for the heads)."""
    R = pkg("host.refine")
    L = pkg("_lib").lib()
    cfg = vae_ref.VaeConfig() if which == "train_py_defaults" else vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="none",
                                                                                       decoder_cat=False)
    model, sd = _room_model(cfg)
    rooms = _random_rooms(16, cfg, seed=3)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    kw = dict(bank=bank, learning_rate=1e-3, image_size=96, iters=4)

    def run(sel, capture=False):
        rb = R.RefineBatch(model, [rooms[i] for i in sel], **kw)
        info = rb.launches()
        losses = rb.run(capture=capture).cpu().numpy().copy()
        out = dict(losses=losses, boxes=[b.cpu().numpy().copy() for b, _ in rb.results()], idx=[i.cpu().numpy().copy() for _, i in rb.results()],
                   z=rb.z.cpu().numpy().copy(), params=rb.params.cpu().numpy().copy(), row0=rb.row0, rows=rb.rows, info=info)
        rb.close()
        return out
    try:
        L.sln_set_deterministic(1)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            full = run(range(16))
            again = run(range(16))
            three = run([4, 9, 15])
            ones = {r: run([r]) for r in (0, 9, 15)}
            graph = run(range(16), capture=True)
            # the loss skips the semantic planes of classes without a visible pixel (SlnRefineLoss::live_planes): the same run
            # with every plane processed must give the same bits
            monkeypatch.setenv("SLN_REFINE_ALL_PLANES", "1")
            every_plane = run(range(16))
            monkeypatch.delenv("SLN_REFINE_ALL_PLANES")
            # the head glue as its own two launches instead of inside the placement launches: the same arithmetic, the same bits
            monkeypatch.setenv("SLN_REFINE_SEPARATE_HEAD", "1")
            separate_head = run(range(16))
            monkeypatch.delenv("SLN_REFINE_SEPARATE_HEAD")
            # the stand-alone SGD step over gradient buffers instead of the step in the wgrads' epilogue: p - step * g as one FMA
            # against -step * g rounded and then added - the last bit of an update, 1e-6 of a parameter after four steps
            monkeypatch.setenv("SLN_REFINE_SEPARATE_SGD", "1")
            separate_sgd = run(range(16))
            monkeypatch.delenv("SLN_REFINE_SEPARATE_SGD")
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    assert full["info"]["single_room_fallbacks"] == 0, full["info"]
    assert np.isfinite(full["losses"]).all()
    moved = sum(len(set(full["losses"][:, r].tolist())) > 1 for r in range(16))
    assert moved >= 12, "only %d of 16 rooms saw a gradient" % moved
    for name, other, sel in [("repeat", again, list(range(16))), ("R=3", three, [4, 9, 15]), ("graph", graph, list(range(16))),
                             ("every plane", every_plane, list(range(16))), ("separate head launches", separate_head, list(range(16)))] + \
                            [("R=1 room %d" % r, o, [r]) for r, o in ones.items()]:
        for j, r in enumerate(sel):
            assert np.array_equal(other["losses"][:, j], full["losses"][:, r]), "%s: losses of room %d" % (name, r)
            assert np.array_equal(other["boxes"][j], full["boxes"][r]) and np.array_equal(other["idx"][j], full["idx"][r]), "%s: layout of room %d" % (name, r)
            a, n = full["row0"][r], full["rows"][r]
            b = other["row0"][j]
            assert np.array_equal(other["z"][b:b + n], full["z"][a:a + n]), "%s: z of room %d" % (name, r)
            assert np.array_equal(other["params"][j], full["params"][r]), "%s: parameters of room %d" % (name, r)
    assert_close(separate_sgd["losses"], full["losses"], "losses, stand-alone SGD step", rtol=1e-5)
    assert_close(separate_sgd["params"], full["params"], "parameters, stand-alone SGD step", rtol=1e-5, atol=1e-7)
    assert not np.array_equal(separate_sgd["params"], sd_flat(model)[None].repeat(16, 0)), "the parameters moved"
    # default mode against the autograd-based one-room loop on its own copy of the checkpoint
    M = pkg("host.Sg2ScVAE_model")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dflt = run(range(16))
        for r in (2, 11):
            m1 = M.Sg2ScVAEModel(**cfg.model_kwargs()); m1.load_state_dict(sd); m1 = m1.cuda().eval()
            rm = rooms[r]
            l1, (b1, i1) = R.finetune_vae_fast(m1, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=4,
                                               bank=bank, learning_rate=1e-3, image_size=96)
            assert_close(dflt["losses"][:, r], l1.cpu().numpy(), "losses of room %d vs finetune_vae_fast" % r, rtol=1e-5)
            assert_close(dflt["boxes"][r], b1.cpu().numpy(), "boxes of room %d" % r, rtol=1e-5, atol=1e-6)
            assert_close(dflt["idx"][r], i1.cpu().numpy(), "angles of room %d" % r, rtol=1e-5, atol=1e-5)
            assert_close(dflt["params"][r], m1.flat_params.detach().cpu().numpy(), "parameters of room %d" % r, rtol=1e-5, atol=1e-7)
    torch.cuda.synchronize()


def test_rooms_in_flight_edge_cases():
    """A batch that mixes an ordinary room, a room whose objects are all of classes the renderer skips (door / window: no visible
    object, only the shell - diff_render.py:93-97), and a two-object room; hipGraph replay of a batch of ONE room; use_attr=False.
    Every room equals its own single-room run bit for bit (deterministic mode) and the skipped-class room keeps a finite loss with
    zero layout gradient."""
    R = pkg("host.refine")
    L = pkg("_lib").lib()
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch", use_attr=False)
    model, sd = _room_model(cfg)
    rooms = _random_rooms(3, cfg, seed=11)
    k = len(rooms[1]["class_names"]) - 1
    rooms[1]["class_names"] = ["door", "window"] * (k // 2) + ["door"] * (k % 2) + ["__room__"]
    r2 = rooms[2]
    keep = [0, 1, len(r2["class_names"]) - 1]
    rooms[2] = dict(objs=r2["objs"][keep], triples=torch.tensor([[0, 3, 1], [0, 0, 2], [1, 0, 2]], device="cuda"), boxes=r2["boxes"][keep],
                    angles=r2["angles"][keep], attributes=r2["attributes"][keep], class_names=[r2["class_names"][i] for i in keep])
    bank = R.MeshBank(FURN, "cuda", seed=3)
    kw = dict(bank=bank, learning_rate=1e-3, image_size=96, iters=3)
    try:
        L.sln_set_deterministic(1)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            rb = R.RefineBatch(model, rooms, **kw)
            full = rb.run().cpu().numpy().copy()
            boxes = [b.cpu().numpy().copy() for b, _ in rb.results()]
            z_all, rows, row0 = rb.z.cpu().numpy().copy(), rb.rows, rb.row0
            rb.close()
            for r in range(3):
                one = R.RefineBatch(model, [rooms[r]], **kw)
                l1 = one.run(capture=(r == 0)).cpu().numpy()
                assert np.array_equal(l1[:, 0], full[:, r]), "room %d alone (capture=%s)" % (r, r == 0)
                assert np.array_equal(one.results()[0][0].cpu().numpy(), boxes[r])
                assert np.array_equal(one.z.cpu().numpy(), z_all[row0[r]:row0[r] + rows[r]])
                one.close()
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    assert np.isfinite(full).all()
    assert len(set(full[:, 1].tolist())) == 1, "a room without a visible object has nothing to optimise: its loss stays put"
    assert len(set(full[:, 0].tolist())) > 1


def test_sparse_scene_image_and_its_flags_describe_the_full_image():
    """sln_scene_forward_live (what RefineBatch renders with): the flags equal sln_scene_live_channels' after a full
    sln_scene_forward of the same faces; planes flagged 3 are the full image's, planes flagged 0 ARE zeros there and planes
    flagged 1 ARE the constant 1 - what the refinement loss assumes without reading them."""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    _lib = pkg("_lib"); L = _lib.lib(); P = _lib.ptr
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch")
    model, sd = _room_model(cfg)
    rooms = _random_rooms(3, cfg, seed=5)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rb = R.RefineBatch(model, rooms, bank=bank, learning_rate=1e-3, image_size=96, iters=2)
        rb.image.fill_(-7.0)                                   # what the sparse pass does not write stays -7
        rb.run(1)
        sp = _lib.current_stream_ptr()
        full = torch.full_like(rb.image, -7.0)
        flags = torch.zeros_like(rb.live)
        _lib.check(L.sln_scene_forward(P(rb.faces), P(rb.cls), rb.R, rb.F2, rb.S, rb.chan.numel(), P(rb.chan), P(rb.dch), 0.1, 0.001, 100.0, 1e-3,
                                       P(rb.scene_ws), P(full), sp), "sln_scene_forward")
        _lib.check(L.sln_scene_live_channels(P(rb.scene_ws), rb.R, rb.F2, rb.S, rb.chan.numel(), P(rb.chan), P(rb.dch), P(flags), sp),
                   "sln_scene_live_channels")
        torch.cuda.synchronize()
        live, img = rb.live.cpu().numpy(), rb.image.cpu().numpy()
        null_mask = rb.null_mask.cpu().numpy()
        rb.close()
    full, flags = full.cpu().numpy(), flags.cpu().numpy()
    assert set(np.unique(flags).tolist()) <= {0, 1, 3}
    n = {k: int((flags == k).sum()) for k in (0, 1, 3)}
    assert n[0] > 0 and n[1] > 0 and n[3] >= 3 * 3, n
    for b in range(flags.shape[0]):
        for ch in range(flags.shape[1]):
            if flags[b, ch] == 0:
                assert not full[b, ch].any(), (b, ch)
            elif flags[b, ch] == 1:
                assert (full[b, ch] == 1.0).all(), (b, ch)
    assert (full != -7.0).all()
    # the null mask the compose kernel hands to the loss (SlnRefineLoss::null_mask): where the depth-hot values of a pixel sum to < 0.5
    assert np.array_equal(null_mask.astype(bool), full[:, 41:].astype(np.float64).sum(1) < 0.5)
    # the batch's own render of the same faces (rb.faces is rewritten by the next iteration's placement only)
    assert np.array_equal(live, flags)
    for b in range(live.shape[0]):
        for ch in range(live.shape[1]):
            if live[b, ch] == 3:
                assert np.array_equal(img[b, ch], full[b, ch]), (b, ch)
            else:
                assert (img[b, ch] == -7.0).all(), (b, ch, live[b, ch])


def test_rooms_in_flight_with_a_recurrent_decoder():
    """gconv_mode='recurrent' applies ONE GraphTripleConv gconv_num_layers times: every weight of it receives that many wgrads per
    backward pass, and with the SGD step in the wgrads' epilogue each of them steps the weight (the sum of the steps is the step of
    the summed gradient).  Rooms in flight equal the autograd one-room loop; deterministic runs are bit-identical per room."""
    R = pkg("host.refine"); M = pkg("host.Sg2ScVAE_model")
    L = pkg("_lib").lib()
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=3, gconv_mode="recurrent", mlp_normalization="batch")
    model, sd = _room_model(cfg)
    rooms = _random_rooms(3, cfg, seed=21)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    kw = dict(bank=bank, learning_rate=1e-3, image_size=96, iters=3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rb = R.RefineBatch(model, rooms, **kw)
        losses = rb.run().cpu().numpy().copy()
        params = rb.params.cpu().numpy().copy()
        res = [(b.cpu().numpy().copy(), i.cpu().numpy().copy()) for b, i in rb.results()]
        rb.close()
        assert np.isfinite(losses).all()
        assert not np.array_equal(params[0], model.flat_params.detach().cpu().numpy()), "the parameters moved"
        for r in (0, 2):
            m1 = M.Sg2ScVAEModel(**cfg.model_kwargs()); m1.load_state_dict(sd); m1 = m1.cuda().eval()
            rm = rooms[r]
            l1, (b1, i1) = R.finetune_vae_fast(m1, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=3,
                                               bank=bank, learning_rate=1e-3, image_size=96)
            assert_close(losses[:, r], l1.cpu().numpy(), "losses of room %d vs finetune_vae_fast" % r, rtol=1e-5)
            assert_close(res[r][0], b1.cpu().numpy(), "boxes of room %d" % r, rtol=1e-5, atol=1e-6)
            assert_close(params[r], m1.flat_params.detach().cpu().numpy(), "parameters of room %d" % r, rtol=1e-5, atol=1e-7)
        try:
            L.sln_set_deterministic(1)
            a = R.RefineBatch(model, rooms, **kw); la = a.run().cpu().numpy().copy(); pa = a.params.cpu().numpy().copy(); a.close()
            b = R.RefineBatch(model, [rooms[1]], **kw); lb = b.run().cpu().numpy().copy(); pb = b.params.cpu().numpy().copy(); b.close()
        finally:
            L.sln_set_deterministic(0)
        assert np.array_equal(la[:, 1], lb[:, 0]) and np.array_equal(pa[1], pb[0])
    torch.cuda.synchronize()


def test_the_side_stream_of_a_caller_stream_overlaps_with_it():
    """csrc/streams.hip: the runtime deals a process's streams to a few hardware queues round-robin and two streams on one queue
    serialise; the library probes, per caller stream, which stream of its pool really runs next to it.  Whatever streams this
    process created before: for several caller streams the chosen side stream passes a fresh probe."""
    _lib = pkg("_lib"); L = _lib.lib()
    import ctypes as C
    junk = [torch.cuda.Stream() for _ in range(5)]          # shift the round-robin
    seen = []
    for _ in range(4):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            torch.zeros(8, device="cuda").add_(1)          # the stream exists on the device
            idx, ov = C.c_int(-1), C.c_int(-1)
            rc = L.sln_debug_side_stream(_lib.current_stream_ptr(), C.byref(idx), C.byref(ov))
            if rc == -3:                                   # SLN_E_STATE: no stream of the pool overlaps with this one
                continue
            _lib.check(rc, "sln_debug_side_stream")
            seen.append((idx.value, ov.value))
    torch.cuda.synchronize()
    if not seen:
        pytest.skip("no two streams of this process overlap (GPU_MAX_HW_QUEUES=1?): the library then forks nothing")
    assert all(0 <= i < 4 for i, _ in seen), seen
    assert all(o == 1 for _, o in seen), "a side stream that does not overlap with its caller stream: %s" % (seen,)
    del junk


def test_rooms_in_flight_at_an_image_size_the_sparse_loss_path_does_not_take():
    """64 x 64 renders are UP-sampled to the 96 x 96 pooled maps: an image pixel feeds more pooled pixels than the register-list
    backward kernel holds, the loss ignores live_planes there (sln_refine_loss_live_ok = 0) - the batch must then render every
    plane (not the sparse scene pass, whose dead planes the loss would read) and still equal the one-room loop."""
    R = pkg("host.refine"); M = pkg("host.Sg2ScVAE_model")
    import ctypes as C
    _lib = pkg("_lib"); L = _lib.lib()
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch")
    model, sd = _room_model(cfg)
    rooms = _random_rooms(2, cfg, seed=31)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    kw = dict(bank=bank, learning_rate=1e-3, image_size=64, iters=2)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rb = R.RefineBatch(model, rooms, **kw)
        took_flags = bool(rb.loss.desc.live_planes)
        assert took_flags == bool(L.sln_refine_loss_live_ok(C.byref(rb.loss.desc)))
        losses = rb.run().cpu().numpy().copy()
        res = [(b.cpu().numpy().copy(), i.cpu().numpy().copy()) for b, i in rb.results()]
        rb.close()
        for r in range(2):
            m1 = M.Sg2ScVAEModel(**cfg.model_kwargs()); m1.load_state_dict(sd); m1 = m1.cuda().eval()
            rm = rooms[r]
            l1, (b1, i1) = R.finetune_vae_fast(m1, rm["objs"], rm["triples"], rm["boxes"], rm["angles"], rm["attributes"], rm["class_names"], iters=2,
                                               bank=bank, learning_rate=1e-3, image_size=64)
            assert_close(losses[:, r], l1.cpu().numpy(), "losses of room %d vs finetune_vae_fast" % r, rtol=1e-5)
            assert_close(res[r][0], b1.cpu().numpy(), "boxes of room %d" % r, rtol=1e-5, atol=1e-6)
    torch.cuda.synchronize()
    assert not took_flags, "expected the all-planes path at this size (if the kernels learnt to take it, this test needs another size)"


@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("edit", ["z", "param"])
def test_first_iterate_size_targets_follow_edits_made_before_the_first_run(edit, capture):
    """The size targets are the FIRST iterate's sizes (testing/test_render_refine.py:319-327), whatever the caller did to z or the
    parameters between construction and the first run(): iteration 0's size term is exactly 0 (the reference's size_loss = 0.0)
    and the targets are that iterate's sizes bit for bit; an edit after iteration 0 leaves them frozen."""
    R = pkg("host.refine")
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch")
    model, _ = _room_model(cfg)
    rooms = _random_rooms(2, cfg, seed=5)
    bank = R.MeshBank(FURN, "cuda", seed=3)
    rb = R.RefineBatch(model, rooms, bank=bank, image_size=96, iters=3)
    try:
        g = torch.Generator(device="cuda").manual_seed(21)
        if edit == "z":
            rb.z.add_(0.05 * torch.randn(rb.z.shape, generator=g, device="cuda"))
        else:                                                  # one row of the box head's first Linear, in every room's copy
            t = dict(model.named_parameters())["box_net.0.weight"]
            off = (t.data_ptr() - model.flat_params.data_ptr()) // 4
            k = t.shape[1]
            row = rb.params[:, off + 3 * k:off + 4 * k]
            row.add_(0.05 * torch.randn(row.shape, generator=g, device="cuda"))
        rb.run(1, capture=capture)
        torch.cuda.synchronize()
        vis = [(r, sc.n_vis) for r, sc in enumerate(rb.scenes) if sc.n_vis]
        assert vis
        assert rb.size_loss.cpu().tolist() == [0.0] * rb.R, "iteration 0 measures its sizes against themselves"
        for r, n in vis:
            assert torch.equal(rb._size_targets[r], rb.sizes[r, :n]), "room %d: the targets are iteration 0's sizes" % r
        frozen = [t.clone() for t in rb._size_targets]
        rb.z.add_(0.05 * torch.randn(rb.z.shape, generator=g, device="cuda"))
        rb.run(1, capture=capture)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(frozen, rb._size_targets)), "targets frozen after iteration 0"
        assert float(rb.size_loss.max()) > 0.0
    finally:
        rb.close()
