"""The refinement pictures on the device (csrc/scene_pictures.hip through host/scene_pictures.py::ScenePictures and
RefineBatch(pictures=...)) against tests/golden/scene_pictures.npz (the reference's save_images / save_label_depth executed from its
source text, tools/gen_golden_scene_pictures.py) and against the torch restatement computed on the CPU.  Every comparison is byte-exact
over every pixel.  The kernels' workgroup covers 1 024 pixels: S = 64 is four workgroups a room."""
import numpy as np
import pytest
import torch

import scene_picture_cases as K
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIELDS = ("depth8", "labels", "rgb", "masks8", "status")


def SP():
    return pkg("host.scene_pictures")


def _quiet_warnings():
    """(without PIL the writers warn and write nothing)"""
    import warnings
    return warnings.catch_warnings(record=True)


def _run(img, live=None, masks=True):
    """-> (ScenePictures, Pictures on the CPU) of one call on the numpy image"""
    B, C, S, _ = img.shape
    sp = SP().ScenePictures(S, batch=B, channels=C, masks=masks, device=DEV)
    got = sp(torch.from_numpy(np.array(img, copy=True)).to(DEV), None if live is None else torch.from_numpy(live).to(DEV))
    torch.cuda.synchronize()
    return sp, SP().Pictures(*[None if t is None else t.cpu().clone() for t in got])


def _same(got, want, what, fields=FIELDS):
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        if w is None or g is None:
            assert g is None and w is None, (what, f)
            continue
        n = int((g != w).sum())
        print("%s %s: %d differing of %d" % (what, f, n, w.numel()))
        assert g.dtype == w.dtype and g.shape == w.shape and n == 0, "%s %s: %d differing" % (what, f, n)


@pytest.mark.parametrize("name", K.FIXTURE_CASES)
def test_fixture_cases(name):
    g = load_golden("scene_pictures")
    img = K.case(name)
    assert K.sha256(img) == bytes(g[name + ":sha256"]).decode()
    _, got = _run(img)
    labels = np.where(g[name + ":flat"] < 0, 0, g[name + ":flat"] + 1).astype(np.uint8)
    want = dict(depth8=g[name + ":depth"], masks8=g[name + ":masks"], labels=labels, rgb=g["palette"][labels])
    if name + ":color" in g.files:
        assert np.array_equal(want["rgb"], g[name + ":color"])
    for f, w in want.items():
        a = getattr(got, f).numpy()
        n = int((a != w).sum())
        print("%s %s: %d differing of %d" % (name, f, n, w.size))
        assert a.shape == w.shape and n == 0, "%s %s: %d differing bytes" % (name, f, n)
    assert got.status.tolist() == [0] * img.shape[0]


def test_channel_forms_agree():
    """the 70-channel tensor and its 41-channel slice give the same pictures; the S = 64 rooms with depth-hot planes behind them"""
    img = K.case("s64_b3_c70")
    assert K.in_domain(img)
    want = SP().scene_pictures_torch(torch.from_numpy(img.copy()))
    _, a = _run(img)
    _, b = _run(np.ascontiguousarray(img[:, :41]))
    _same(a, want, "70 channels")
    _same(b, want, "41 channels")


def test_live_flags():
    dirty, live, clean = K.live_case()
    want = SP().scene_pictures_torch(torch.from_numpy(clean))
    _, a = _run(dirty, live)
    _same(a, want, "flags on the dirty image")
    _, b = _run(clean, None)
    _same(b, want, "live=None on the cleaned image")


def test_status_bits_inside_a_batch():
    img = K.status_case()
    want = SP().scene_pictures_torch(torch.from_numpy(img))
    assert want.status.tolist() == [0, 1, 2, 0]
    _, got = _run(img)
    _same(got, want, "status batch")
    assert int(got.depth8[1].max()) == 0 and int(got.depth8[2].max()) == 0 and int(got.depth8[0].max()) == 255


def test_null_outputs_are_not_written():
    L = pkg("_lib")
    img = K.case("s12_c70")
    B, C, S, _ = img.shape
    _, full = _run(img)
    x = torch.from_numpy(img.copy()).to(DEV)
    # masks=False: no masks buffer exists, the other outputs are the same
    sp = SP().ScenePictures(S, batch=B, channels=C, masks=False, device=DEV)
    got = sp(x)
    torch.cuda.synchronize()
    assert got.masks8 is None
    _same(SP().Pictures(*[None if t is None else t.cpu() for t in got]), full, "masks=False", ("depth8", "labels", "rgb", "status"))
    # a masks buffer the call is not given stays as it was; then depth only: labels and rgb keep their sentinels too
    sp = SP().ScenePictures(S, batch=B, channels=C, masks=True, device=DEV)
    sp.masks8.fill_(0xA5)
    sp.into(x, None, sp.depth8, sp.labels, sp.rgb, None, sp.status)
    torch.cuda.synchronize()
    assert bool((sp.masks8 == 0xA5).all())
    assert torch.equal(sp.depth8.cpu(), full.depth8) and torch.equal(sp.labels.cpu(), full.labels) and torch.equal(sp.rgb.cpu(), full.rgb)
    sp.labels.fill_(0x5A); sp.rgb.fill_(0x5A); sp.depth8.fill_(0x5A); sp.status.fill_(-1)
    sp.into(x, None, sp.depth8, None, None, None, sp.status)
    torch.cuda.synchronize()
    assert torch.equal(sp.depth8.cpu(), full.depth8) and sp.status.tolist() == [0] * B
    assert bool((sp.labels == 0x5A).all()) and bool((sp.rgb == 0x5A).all()) and bool((sp.masks8 == 0xA5).all())
    assert L.lib().sln_scene_pictures_workspace_bytes(B, S) == 8 * B


def test_repeatable_and_capturable():
    img = K.case("s64_b3_c70")
    x = torch.from_numpy(img.copy()).to(DEV)
    B, C, S, _ = img.shape
    sp = SP().ScenePictures(S, batch=B, channels=C, masks=True, device=DEV)
    first = [t.clone() for t in sp(x)]
    second = [t.clone() for t in sp(x)]
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a linear capture: three kernel nodes
        sp(x)
    for _ in range(2):
        for t in (sp.depth8, sp.labels, sp.rgb, sp.masks8):
            t.fill_(0x77)
        sp.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (sp.depth8, sp.labels, sp.rgb, sp.masks8, sp.status)):
            assert torch.equal(a, b)


def test_refusals_launch_nothing():
    S_, L = SP(), pkg("_lib")
    with pytest.raises(ValueError):
        S_.ScenePictures(6, device=DEV)
    img = K.case("s12_c70")
    B, C, S, _ = img.shape
    sp = S_.ScenePictures(S, batch=B, channels=C, masks=True, device=DEV)
    outs = (sp.depth8, sp.labels, sp.rgb, sp.masks8)
    for t in outs:
        t.fill_(0xC3)
    sp.status.fill_(-5)
    x = torch.from_numpy(img.copy())
    for bad in (x, x.to(DEV).double(), x.to(DEV)[:, :41].contiguous(), x.to(DEV)[..., :8].contiguous(), x.to(DEV).half()):
        with pytest.raises(ValueError):
            sp(bad)
    with pytest.raises(ValueError):
        sp(x.to(DEV), live=torch.full((B, C), 3, dtype=torch.int32, device=DEV))
    # the C entry itself: S = 6 (and the other geometry rules) with every pointer valid
    lib, P = L.lib(), L.ptr
    six = torch.zeros(1, 41, 6, 6, device=DEV)
    for Bq, Cq, Sq in ((1, 41, 6), (0, 41, 12), (1, 42, 12)):
        rc = lib.sln_scene_pictures(P(six), Bq, Cq, Sq, None, P(sp._palette), P(sp._ws), P(sp.depth8), P(sp.labels), P(sp.rgb), P(sp.masks8),
                                    P(sp.status), L.current_stream_ptr())
        assert rc == -2, (Bq, Cq, Sq, rc)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 0xC3).all())
    assert sp.status.tolist() == [-5] * B


def test_save_images_and_save_label_depth_keep_the_references_call_shape(tmp_path):
    g = load_golden("scene_pictures")
    name = "s256_c70"
    img = torch.from_numpy(K.case(name).copy())                                # a CPU tensor, as the reference's callers hold
    folder = str(tmp_path / "pictures")
    with _quiet_warnings():
        pics = SP().save_images(img, save_semantic=True, folder_name=folder, prefix="000")
        flat = torch.from_numpy(g[name + ":flat"].astype(np.float32))[None]     # [1, 1, S, S]: class 0..39, -100 where empty
        both = SP().save_label_depth(flat, img[:, :1].to(DEV), folder_name=folder, prefix="target")
    assert pics.depth8.device.type == "cuda"
    assert np.array_equal(pics.depth8.cpu().numpy(), g[name + ":depth"]) and np.array_equal(pics.masks8.cpu().numpy(), g[name + ":masks"])
    assert np.array_equal(both.rgb.cpu().numpy(), g[name + ":color"]) and np.array_equal(both.depth8.cpu().numpy(), g[name + ":depth"])
    try:
        from PIL import Image
    except ImportError:
        return
    import os
    want = ["000_depth.png", "target_depth.png", "target_class_color.png"] + ["000_%s.png" % n for n in SP().NYU_CLASS]
    assert sorted(os.listdir(folder)) == sorted(want)
    assert np.array_equal(np.asarray(Image.open(os.path.join(folder, "000_depth.png"))), g[name + ":depth"][0])
    assert np.array_equal(np.asarray(Image.open(os.path.join(folder, "target_class_color.png")).convert("RGB")), g[name + ":color"][0])
    assert np.array_equal(np.asarray(Image.open(os.path.join(folder, "000_floor mat.png"))), g[name + ":masks"][0, 19])


# ------------------------------------------------------------------------------------------------------------------------------
# RefineBatch(pictures=...)
# ------------------------------------------------------------------------------------------------------------------------------
def _refine(pictures, iters=3):
    """the two rooms of the refine_loop fixture -> what the run leaves behind (CPU tensors)"""
    import test_refine_report_gpu as RR
    R = pkg("host.refine")
    g = load_golden("refine_loop")
    model = RR._loop_model(g, "refine_loop")
    rooms = RR._loop_rooms(g, [0, 1])
    rb = R.RefineBatch(model, rooms, bank=RR._bank(g), image_size=RR.LOOP_IMAGE, iters=iters, pictures=pictures)
    snaps = {}
    try:
        for i, r in enumerate([0, 1]):
            a, n = rb.row0[i], rb.rows[i]
            rb.z[a:a + n] = torch.from_numpy(g["room%d:z0" % r]).to(DEV)
        for k in range(iters):
            rb.run(1)
            torch.cuda.synchronize()
            snaps[k] = (rb.image.cpu().clone(), rb.live.cpu().clone())
        out = dict(losses=rb.losses.cpu().clone(), boxes=rb.boxes.cpu().clone(), idx=rb.idx.cpu().clone(), snaps=snaps,
                   has=hasattr(rb, "pictures") or hasattr(rb, "target_pictures"))
        if pictures is not None:
            out["pictures"] = R.PictureSet(*[t.cpu().clone() for t in rb.pictures[:4]], rb.pictures.iterations)
            out["target_pictures"] = SP().Pictures(*[None if t is None else t.cpu().clone() for t in rb.target_pictures])
            # the targets, rendered again the way the set-up renders them
            with torch.no_grad():
                out["targets"] = torch.cat([sc.render(rm["boxes"], rm["angles"].float())[0] for sc, rm in zip(rb.scenes, rooms)], 0).cpu()
    finally:
        rb.close()
    return out


def test_refine_batch_pictures_at_the_ends():
    L = pkg("_lib").lib()
    L.sln_set_deterministic(1)
    try:
        none = _refine(None)
        ends = _refine("ends")
    finally:
        L.sln_set_deterministic(0)
    assert not none["has"]
    pics = ends["pictures"]
    assert pics.iterations == (0, 2) and pics.depth8.shape == (2, 2, 96, 96) and pics.rgb.shape == (2, 2, 96, 96, 3)
    for j, k in enumerate(pics.iterations):
        image, live = ends["snaps"][k]
        print("iteration %d: planes flagged dead per room %s" % (k, ((live & 1) == 0).sum(1).tolist()))
        want = SP().scene_pictures_torch(image, live, masks=False)
        got = SP().Pictures(pics.depth8[j], pics.labels[j], pics.rgb[j], None, pics.status[j])
        _same(got, want, "iteration %d" % k)
        assert int(want.labels.max()) > 0 and int(want.depth8.max()) == 255
    want = SP().scene_pictures_torch(ends["targets"], masks=False)
    _same(ends["target_pictures"], want, "target")
    for k in ("losses", "boxes", "idx"):
        assert torch.equal(none[k], ends[k]), k


def test_refine_batch_pictures_arguments():
    import test_refine_report_gpu as RR
    R = pkg("host.refine")
    g = load_golden("refine_loop")
    model = RR._loop_model(g, "refine_loop")
    rooms, bank = RR._loop_rooms(g, [0]), RR._bank(g)
    for bad in ("some", [5]):
        with pytest.raises(ValueError):
            R.RefineBatch(model, rooms, bank=bank, image_size=RR.LOOP_IMAGE, iters=4, pictures=bad)
    rb = R.RefineBatch(model, rooms, bank=bank, image_size=RR.LOOP_IMAGE, iters=4, pictures=[2])
    try:
        with pytest.raises(ValueError):
            rb.run(capture=True)                                              # one graph for every iteration: 'all' or None
    finally:
        rb.close()
    L = pkg("_lib").lib()
    L.sln_set_deterministic(1)
    try:
        eager = R.finetune_vae_fast_batch(model, rooms, iters=3, bank=bank, image_size=RR.LOOP_IMAGE, pictures="all")
        graph = R.finetune_vae_fast_batch(model, rooms, iters=3, bank=bank, image_size=RR.LOOP_IMAGE, pictures="all", capture=True)
    finally:
        L.sln_set_deterministic(0)
    assert len(eager) == 3 and eager[2][0].iterations == (0, 1, 2)
    # a replayed iteration's pictures are those of its own image: iteration 0 (eager in both) equal, the others drawn and not blank
    assert torch.equal(eager[2][0].depth8[0], graph[2][0].depth8[0]) and torch.equal(eager[2][1].rgb, graph[2][1].rgb)
    assert int(graph[2][0].depth8[2].max()) == 255 and int(graph[2][0].labels[2].max()) > 0
