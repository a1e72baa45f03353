"""3-D drawing on the device (csrc/draw3d.hip through host/draw3d.py; run with -m gpu), at operand level: ``sln_draw3d`` on the device's
own faces and maps against ``draw3d_torch`` in float64 on those same operands copied to the host - only the shading arithmetic differs -,
hand-made operands that need no renderer, ``Draw3D`` end to end, repeated calls and graph replays, and ``render_test_3d``."""
import numpy as np
import pytest
import torch

import draw3d_cases as DC
import shade_view_cases as CS
from conftest import pkg
from gpu_util import _lib, _sync

pytestmark = pytest.mark.gpu

# Largest |fp32 - fp64| / max(1, |fp64|) of ``linear`` over the safe hit samples of every room case of draw3d_cases.ROOMS, both precisions
# of draw3d_torch run on the host on the same operands: measured 4.717e-07 (tests/test_draw3d_host.py prints it per case and holds this
# constant to it).  The kernel does the same operations with FMA contraction and in another order - its only licence - and is allowed
# four times that figure: 1.92e-06.
FP32_TORCH_ERR = 4.8e-7
KERNEL_ALLOWANCE = 4.0 * FP32_TORCH_ERR


def _launch(D, dev, k, background, shadows=True):
    """``sln_draw3d`` on the device operands ``dev`` -> (picture, linear) on the host; buffers prefilled with what no kernel writes"""
    R, F = dev["face_label"].shape
    S = dev["face_index"].shape[1]
    ws = torch.empty(int(pkg("_lib").lib().sln_draw3d_workspace_bytes(R, F)) // 4, dtype=torch.float32, device="cuda")
    picture = torch.full((R, S // k, S // k, 3), 77, dtype=torch.uint8, device="cuda")
    linear = torch.full((R, S, S, 3), -777.25, dtype=torch.float32, device="cuda")
    D.draw3d_launch(dev["faces_xyz"], dev["face_index"], dev["depth"], dev["face_label"], dev["chosen"], dev["K"], dev["light_cam"], D.albedo_table("cuda"),
                    k, ws, picture, linear, background=background, shadows=shadows)
    _sync("sln_draw3d at k = %d" % k)
    return picture.cpu(), linear.cpu()


def _hold(D, name, op, want, k, picture, linear):
    """the checks every operand case shares"""
    err, unsafe, hits = DC.linear_error(linear, want)
    print("%s k=%d: kernel against fp64 on %d hit samples, largest |d| / max(1, |want|) = %.3e (allowed %.3e; fp32 torch %.3e); unsafe %.4f %%"
          % (name, k, hits, err, KERNEL_ALLOWANCE, FP32_TORCH_ERR, 100 * unsafe))
    assert err <= KERNEL_ALLOWANCE and unsafe <= DC.UNSAFE_CAP
    bg = torch.tensor(op["background"], dtype=torch.float32)
    assert bool((linear[~want["hit"]] == bg).all()), "background samples are exactly the background"
    own = D.encode_picture(linear.double(), k)
    assert picture.shape == own.shape and int((picture.int() - own.int()).abs().max()) <= 1, "picture against the encoded box filter of the device's linear"


def _device(op):
    f = lambda t, dt: t.to(dt).contiguous().cuda()
    return dict(faces_xyz=f(op["faces_xyz"], torch.float32), face_index=f(op["face_index"], torch.int32), depth=f(op["depth"], torch.float32),
                face_label=f(op["face_label"], torch.uint8), chosen=f(op["chosen"], torch.int64), K=f(op["K"], torch.float32),
                light_cam=f(op["light_cam"], torch.float32))


@pytest.mark.parametrize("name", list(DC.HAND))
def test_hand_made_operands(name):
    _lib()
    D = pkg("host.draw3d")
    op, want = DC.operands(name), DC.want(name)
    dev = _device(op)
    for k in sorted(set(op["ks"]) | {1}):
        picture, linear = _launch(D, dev, k, op["background"])
        _hold(D, name, op, want, k, picture, linear)
    if name == "label_above_40":
        big = (op["face_label"][0][op["face_index"][0].clamp(min=0).long()] > 40) & want["hit"][0]
        assert int(big.sum()) > 20 and bool((linear[0][big] == 0).all()), "a byte above 40 reads albedo entry 0"
    if name == "lamp_behind":
        assert torch.allclose(linear.double()[want["hit"]], want["linear"][want["hit"]], rtol=1e-6)
    if name == "occluder":
        off_p, off_l = _launch(D, dev, 1, op["background"], shadows=False)
        _hold(D, name + " without shadows", op, DC.reference(op, 1, shadows=False), 1, off_p, off_l)
        assert not torch.equal(off_l, linear)


@pytest.mark.parametrize("name", list(DC.ROOMS))
def test_rooms_at_operand_level(name):
    _lib()
    SH, D = pkg("host.shade"), pkg("host.draw3d")
    c = CS.case(name)
    r = SH.ViewRenderer(CS.bank("cuda"), size=c["S"], views=c["V"], batch=c["R"], near=c["near"], far=DC.FAR)
    draw = D.Draw3D(r, percentage=100, linear=True)
    picture, status = draw.draw3d(c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"], draws=c["draws"].cuda())
    _sync("Draw3D %dx%d views at %d" % (c["R"], c["V"], c["S"]))
    dev = dict(faces_xyz=r.faces_xyz, face_index=r.face_index, depth=r._raster_depth, face_label=r.face_label, chosen=r.chosen, K=draw.K,
               light_cam=draw.light_cam)
    op = {key: t.cpu() for key, t in dev.items()}
    op.update(light_cam=op["light_cam"].double(), background=(0.0, 0.0, 0.0), S=c["S"])
    # the lamp the device formed against :405 through the float64 cameras
    host = DC.operands(name)
    if torch.equal(op["chosen"], host["chosen"]):
        assert float((op["light_cam"] - host["light_cam"]).abs().max()) < 1e-4
    want = DC.reference(op, 1)
    _hold(D, name, op, want, 1, picture.cpu(), draw.linear.cpu())
    for k in DC.ROOMS[name]:
        pk, lk = _launch(D, dev, k, op["background"])
        _hold(D, name, op, want, k, pk, lk)
        assert k > 1 or (torch.equal(pk, picture.cpu()) and torch.equal(lk, draw.linear.cpu()))
    if name == "every_face_culled":
        assert not bool(want["hit"].any()) and bool((draw.linear == 0).all()) and bool((picture == 0).all()) and status.tolist() == [1]
    else:
        assert bool(want["hit"].any()) and int(picture.max()) > 0
    if name == "five_views":
        dark = float((want["hit"] & ~want["visible"]).sum()) / float(want["hit"].sum())
        assert 0.02 <= dark <= 0.98


def _room_64():
    return dict(CS.case("five_views"), S=64)


def test_draw3d_end_to_end_on_one_room():
    _lib()
    SH, D = pkg("host.shade"), pkg("host.draw3d")
    c = _room_64()
    bnk = CS.bank("cuda")
    args = (c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"])
    r = SH.ViewRenderer(bnk, size=c["S"], views=c["V"], batch=1, near=c["near"], far=DC.FAR)
    draw = D.Draw3D(r, linear=True)
    with pytest.raises(ValueError, match="last"):
        draw.draw3d()
    picture, status = draw.draw3d(*args, draws=c["draws"].cuda())
    _sync("Draw3D end to end")
    assert draw.k == 4 and picture.shape == (1, 16, 16, 3) and picture.dtype == torch.uint8 and picture.is_cuda and status.tolist() == [0]
    op = dict(faces_xyz=r.faces_xyz.cpu(), face_index=r.face_index.cpu(), depth=r._raster_depth.cpu(), face_label=r.face_label.cpu(),
              chosen=r.chosen.cpu(), K=draw.K.cpu(), light_cam=draw.light_cam.cpu().double(), background=(0.0, 0.0, 0.0), S=c["S"])
    want = DC.reference(op, 4)
    _hold(D, "five_views at 64", op, want, 4, picture.cpu(), draw.linear.cpu())
    b = int(r.chosen[0])
    seen = op["face_label"][0][op["face_index"][b].clamp(min=0).long()][want["hit"][0]]
    assert len(set(seen.tolist())) >= 4, "at least four distinct albedos"
    lit, dark = want["hit"] & want["visible"], want["hit"] & ~want["visible"]
    assert int(lit.sum()) > 50 and int(dark.sum()) > 50
    # the renderer's buffers are those of a renderer that was never drawn from
    r2 = SH.ViewRenderer(bnk, size=c["S"], views=c["V"], batch=1, near=c["near"], far=DC.FAR)
    r2(*args, draws=c["draws"].cuda())
    _sync("a renderer that is not drawn from")
    for key in ("faces_xyz", "face_index", "_raster_depth", "face_label", "labels_all", "depth_all", "labels", "depth", "chosen", "status", "sums", "counts"):
        a, b2 = getattr(r, key), getattr(r2, key)
        assert torch.equal(a.contiguous().view(torch.uint8), b2.contiguous().view(torch.uint8)), key
    # drawing again from what is left: the same bytes
    again, _ = draw.draw3d()
    _sync("draw3d() without arguments")
    assert torch.equal(again.cpu(), picture.cpu())


def test_second_call_and_graph_replays_give_the_same_bytes_and_follow_chosen_and_draws():
    _lib()
    SH, D = pkg("host.shade"), pkg("host.draw3d")
    c = _room_64()
    r = SH.ViewRenderer(CS.bank("cuda"), size=c["S"], views=c["V"], batch=1, near=c["near"], far=DC.FAR)
    draw = D.Draw3D(r, linear=True)
    args = (c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"])
    draws = c["draws"].cuda()

    def reference():
        op = dict(faces_xyz=r.faces_xyz.cpu(), face_index=r.face_index.cpu(), depth=r._raster_depth.cpu(), face_label=r.face_label.cpu(),
                  chosen=r.chosen.cpu(), K=draw.K.cpu(), light_cam=draw.light_cam.cpu().double(), background=(0.0, 0.0, 0.0), S=c["S"])
        return op, DC.reference(op, 4)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draw.draw3d(*args, draws=draws)
        torch.cuda.synchronize()
        first = [t.clone() for t in (draw.picture, draw.linear)]
        draw.draw3d(*args, draws=draws)
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    _sync("two eager calls")
    assert torch.equal(first[0], draw.picture) and torch.equal(first[1].view(torch.int32), draw.linear.view(torch.int32))
    pkg("_lib").lib().sln_set_deterministic(1)
    try:
        draw.draw3d()
        _sync("a call in deterministic mode")
    finally:
        pkg("_lib").lib().sln_set_deterministic(0)
    assert torch.equal(first[0], draw.picture) and torch.equal(first[1].view(torch.int32), draw.linear.view(torch.int32))
    whole, light = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(whole):
        draw.draw3d(*args, draws=draws)
    with torch.cuda.graph(light):
        draw.draw3d()
    for graph in (whole, whole, light):
        draw.picture.zero_(); draw.linear.zero_()
        graph.replay()
        _sync("replay of the drawing")
        assert torch.equal(first[0], draw.picture) and torch.equal(first[1].view(torch.int32), draw.linear.view(torch.int32))
    # another choice, set on the device: the lighting graph follows it and matches the reference again
    was = int(r.chosen[0])
    r.chosen.fill_((was + 1) % c["V"])
    light.replay()
    _sync("replay with another choice")
    assert not torch.equal(first[0], draw.picture)
    op, want = reference()
    assert op["chosen"].tolist() == [(was + 1) % c["V"]]
    _hold(D, "another choice", op, want, 4, draw.picture.cpu(), draw.linear.cpu())
    # other draws through the whole graph: read on the device
    draws.copy_(torch.flip(draws, [1]))
    whole.replay()
    _sync("replay with other draws")
    assert not torch.equal(first[1], draw.linear)
    op, want = reference()
    _hold(D, "other draws", op, want, 4, draw.picture.cpu(), draw.linear.cpu())


def test_render_test_3d_writes_the_references_files(tmp_path):
    from PIL import Image
    import test_draw3d_host as H
    _lib()
    D = pkg("host.draw3d")
    data = H._tool().two_rooms()
    out = str(tmp_path / "rendered")
    paths = D.render_test_3d(data, CS.bank("cuda"), out, vocab=CS.VOCAB, size=64, rng=torch.Generator(device="cuda").manual_seed(3))
    _sync("render_test_3d")
    import os
    assert [os.path.basename(p) for p in paths] == D.picture_names(data) and len(paths) == 8 and sorted(os.listdir(out)) == sorted(D.picture_names(data))
    pics = [np.asarray(Image.open(p)) for p in paths]
    assert all(p.shape == (16, 16, 3) and p.dtype == np.uint8 for p in pics) and any(int(p.max()) > 0 for p in pics)
    assert not np.array_equal(pics[0], pics[1])
