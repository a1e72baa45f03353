"""Viewpoint render on the device (csrc/shade_view.hip through host/shade.py; run with -m gpu), at operand level: the placing and
projecting kernel against the float64 restatement, the compose kernels exactly against the rasterizer's C restatement run on the device's
own faces, hand-made maps, and ``shade_layouts`` end to end on one small room."""
import numpy as np
import pytest
import torch

import shade_view_cases as CS
from conftest import pkg
from gpu_util import _lib, _sync

pytestmark = pytest.mark.gpu

# Largest |fp32 - fp64| / max(1, |fp64|) over the kept faces of every case of shade_view_cases.CASES, with both restatements run in torch
# on the host: measured 8.307e-06 (tests/test_shade_view_host.py prints it per case and holds this constant to it).  The kernel does the
# same operations with FMA contraction and in another order - its only licence - and is allowed four times that figure: 3.36e-05.
FP32_TORCH_ERR = 8.4e-6
KERNEL_ALLOWANCE = 4.0 * FP32_TORCH_ERR
FAR = 100.0


def _bits(a):
    return a.contiguous().view(torch.int32)


def _render(SH, bnk, c, **kw):
    r = SH.ViewRenderer(bnk, size=c["S"], views=c["V"], batch=c["R"], near=c["near"], far=FAR, **kw)
    out = r(c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"], draws=c["draws"].cuda())
    _sync("ViewRenderer %dx%d views at %d" % (c["R"], c["V"], c["S"]))
    return r, out


@pytest.mark.parametrize("name", [c[0] for c in CS.CASES])
def test_place_project_and_compose_at_operand_level(name):
    from oracle import raster_ref
    _lib()
    SH = pkg("host.shade")
    c = CS.case(name)
    r, (labels, depth, chosen, status) = _render(SH, CS.bank("cuda"), c)
    want = CS.torch_route(SH, CS.bank("cpu"), c, torch.float64)
    F = want["faces_xyz"].shape[1]
    assert r.F == F == max(c["rows"]) * 108 + 360 and r.faces_xyz.shape == (c["R"] * c["V"], F, 3, 3)
    # --- sln_view_place_project against the float64 restatement
    fx, fl = r.faces_xyz.cpu(), r.face_label.cpu()
    assert torch.equal(fl, want["face_label"]), "%d class bytes differ" % int((fl != want["face_label"]).sum())
    err, flips = CS.face_error(fx, want["faces_xyz"])
    print("%s: kernel against fp64, largest |d| / max(1, |want|) = %.3e (allowed %.3e; fp32 torch %.3e)" % (name, err, KERNEL_ALLOWANCE, FP32_TORCH_ERR))
    assert flips == 0 and err <= KERNEL_ALLOWANCE
    live = ~(fx == 0).all(-1).all(-1)
    if name == "every_face_culled":
        assert not bool(live.any()) and bool((labels == 0).all()) and status.tolist() == [1]
    if name == "no_visible_row":
        assert not bool(live[:, :F - 360].any()) and bool(live[:, F - 360:].any()) and bool((fl[:, :F - 360] == 0).all())
    if c["R"] == 17:                                                # padded rows: the slots past a room's rows are empty
        for room, n in enumerate(c["rows"]):
            assert not bool(live[room, (n - 1) * 108:F - 360].any())
    # --- the compose kernels, exactly: the rasterizer's C restatement on the device's own faces
    fi, _, dep = raster_ref.nmr_forward(fx.numpy(), c["S"], c["near"], FAR)
    lab_w, dep_w, sums_w, counts_w = SH.compose_torch(torch.from_numpy(fi), torch.from_numpy(dep), fl, c["V"])
    assert torch.equal(r.labels_all.cpu(), lab_w)
    assert torch.equal(_bits(r.depth_all.cpu()), _bits(dep_w))
    hit = torch.flip(r.face_index.cpu(), [1]) >= 0
    flipped = torch.flip(r._raster_depth.cpu(), [1])
    assert torch.equal(_bits(r.depth_all.cpu())[hit], _bits(flipped)[hit]) and bool((r.depth_all.cpu()[~hit] == 1e10).all())
    assert torch.equal(r.counts.cpu(), counts_w) and torch.allclose(r.sums.cpu(), sums_w, rtol=1e-12, atol=0)
    chosen_w, status_w = SH.choose_view(sums_w.reshape(c["R"], c["V"]), counts_w.reshape(c["R"], c["V"]))
    assert torch.equal(chosen.cpu(), chosen_w) and torch.equal(status.cpu(), status_w)
    pick = torch.arange(c["R"]) * c["V"] + chosen_w
    assert torch.equal(labels.cpu(), lab_w[pick]) and torch.equal(_bits(depth.cpu()), _bits(dep_w[pick]))
    if name not in ("every_face_culled",):
        assert bool((lab_w > 0).any()) and int(counts_w.min()) > 0


def test_a_bank_with_shell_meshes_binds_its_shell_on_the_host():
    _lib()
    SH, RF = pkg("host.shade"), pkg("host.refine")
    c = CS.case("five_views")
    c["objs"] = torch.where((c["objs"] == 1) | (c["objs"] == 3), c["objs"], torch.zeros_like(c["objs"]))
    ext = c["boxes"][-1, 3:].tolist()
    r = SH.ViewRenderer(CS.shell_bank("cuda"), size=c["S"], views=c["V"], batch=1, near=c["near"], far=FAR)
    args = (c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"])
    with pytest.raises(pkg("_lib").SlnError, match="bind_shell"):
        r(*args, draws=c["draws"].cuda())
    r.bind_shell([ext])
    r(*args, draws=c["draws"].cuda())
    _sync("ViewRenderer with a bound shell")
    cpu_bank = CS.shell_bank("cpu")
    tables, bind = SH.BankTables.of(cpu_bank, "cpu"), SH.Binding(c["rows"], None, "cpu")
    rt = SH.row_tables(tables, bind, c["boxes"].double(), c["angles"], c["objs"], None, torch.float64)
    d = c["draws"].double()
    K, Rm, t = SH.shade_camera(rt["ext"][:, None, :].expand(1, c["V"], 3), d[..., 0], d[..., 1], c["S"])
    want, want_label = SH.place_project_torch(tables, rt, RF.place_shell(cpu_bank, ext)[None], K, Rm, t, c["S"], c["near"])
    err, flips = CS.face_error(r.faces_xyz.cpu(), want)
    print("bound shell: kernel against fp64 %.3e (allowed %.3e)" % (err, KERNEL_ALLOWANCE))
    assert torch.equal(r.face_label.cpu(), want_label) and flips == 0 and err <= KERNEL_ALLOWANCE
    assert 2 in set(torch.unique(r.labels_all).tolist())            # (the view looks down: the floor is what it surely sees)


def test_compose_on_hand_made_maps():
    """background everywhere; a label-0 face in front of a labelled one (its pixels read 0, its depth counts); entries at and above 1e5;
    a face index past the table (background); sums that are exact in float64 in any order, so the strict threshold holds on the device"""
    _lib()
    SH = pkg("host.shade")
    R, V, S, F = 2, 3, 33, 5
    rng = np.random.default_rng(3)
    face_label = torch.tensor([[0, 4, 1, 0, 2], [7, 0, 0, 3, 1]], dtype=torch.uint8)
    fi = torch.from_numpy(rng.integers(-1, F, size=(R * V, S, S)).astype(np.int32))
    dep = torch.from_numpy((rng.integers(1, 64, size=(R * V, S, S)) / 8.0).astype(np.float32))
    fi[0] = -1                                                       # view 0 of room 0: nothing hit
    dep[1, :4] = torch.tensor([1e5, 2e5, 99999.0, 1e5])[:, None]     # at, above and just below 1e5
    fi[1, :4] = 1
    fi[2, 5] = F; fi[2, 6] = F + 1000                                # outside the table: background
    fi[4], dep[4] = 3, 0.75                                          # room 1, view 1: mean exactly 0.75
    fi[3, :, :] = 0; dep[3] = 0.5                                    # room 1, view 0: a class-7 surface at 0.5
    dev = lambda t: t.cuda()
    B = R * V
    out = dict(labels=torch.full((B, S, S), 9, dtype=torch.uint8).cuda(), depth=torch.full((B, S, S), -1.0).cuda(),
               sums=torch.full((B,), -1.0, dtype=torch.float64).cuda(), counts=torch.full((B,), -1, dtype=torch.int64).cuda())
    ws = torch.empty(int(pkg("_lib").lib().sln_view_compose_workspace_bytes(B)) // 8, dtype=torch.int64).cuda()
    SH.compose(dev(fi), dev(dep), dev(face_label), V, ws, out["labels"], out["depth"], out["sums"], out["counts"])
    _sync("sln_view_compose on hand-made maps")
    lab_w, dep_w, sums_w, counts_w = SH.compose_torch(fi, dep, face_label, V)
    assert torch.equal(out["labels"].cpu(), lab_w) and torch.equal(_bits(out["depth"].cpu()), _bits(dep_w))
    assert torch.equal(out["counts"].cpu(), counts_w) and torch.equal(out["sums"].cpu(), sums_w), "sums of multiples of 1/8 are exact in any order"
    assert counts_w[0] == 0 and sums_w[0] == 0 and bool((lab_w[0] == 0).all()) and bool((dep_w[0] == 1e10).all())
    # image row order: raster row 0 is the picture's last row
    assert dep_w[1, S - 1, 0] == 1e5 and dep_w[1, S - 2, 0] == 2e5 and counts_w[1] == int((fi[1] >= 0).sum()) - 3 * S
    assert bool((lab_w[2, S - 6] == 0).all()) and bool((dep_w[2, S - 7] == 1e10).all())
    assert bool((lab_w[3] == 7).all()) and bool((lab_w[4] == 3).all())
    # the choice on the device's sums: strict > at an exactly representable mean
    sums, counts = out["sums"].reshape(R, V), out["counts"].reshape(R, V)
    assert float(sums[1, 1] / counts[1, 1]) == 0.75
    chosen, status = SH.choose_view(sums, counts, 0.75)
    assert chosen[1].item() == 2 and status.tolist() == [0, 0]       # views 0 (0.5) and 1 (0.75, not above) fail, view 2 passes
    chosen, status = SH.choose_view(sums, counts, 0.7499999)
    assert chosen[1].item() == 1
    assert chosen[0].item() >= 1, "a view in which nothing was hit is never accepted"


def _room_128():
    """one small room for the end-to-end run: six objects of four classes, two of them sharing a model"""
    c = CS.case("five_views")
    c = dict(c, S=128)
    return c


def _clean_outputs(differ, S, size, width):
    """output pixels of the S -> size resize none of whose taps (a band of ``width`` input pixels) touches a pixel where the class images differ"""
    import torch.nn.functional as Fn
    k = 2 * width + 1
    grown = Fn.max_pool2d(differ[None, None].float(), k, stride=1, padding=width)[0, 0]
    return Fn.max_pool2d(grown[None, None], S // size)[0, 0] == 0


def test_shade_layouts_end_to_end_on_one_room():
    """Class image against views_torch's float64 route: at most 0.5 % of the pixels differ (a condition on the room, checked for the float32
    host route first).  The 41-channel input against ``build_input`` of the float64 route's planes on the output pixels whose taps see
    agreeing pixels only: class channels to ``test_spade_input``'s bound; the depth channel to four times what the float32 HOST route shows
    there (printed)."""
    from oracle import raster_ref, spade_ref
    from oracle.gen_golden_spade import CASES
    _lib()
    SH, SI, G4 = pkg("host.shade"), pkg("host.spade_input"), pkg("host.SPADE_related")
    c = _room_128()
    S, cap = c["S"], 0.005
    cpu_bank = CS.bank("cpu")
    w64 = CS.torch_route(SH, cpu_bank, c, torch.float64, raster_ref.nmr_forward)
    w32 = CS.torch_route(SH, cpu_bank, c, torch.float32, raster_ref.nmr_forward)
    frac32 = float((w32["labels"] != w64["labels"]).float().mean())
    assert w32["chosen"].tolist() == w64["chosen"].tolist() and frac32 <= cap, "the room does not meet the test's condition: %.4f" % frac32
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    G = G4.SPADEGenerator4(cfg.semantic_nc, cfg.target_nc, cfg.nz, cfg.ngf, 'spectralspadelayer3x3', cfg.crop_size, 'normal')
    G.load_state_dict(spade_ref.init_state(cfg, seed=7)); G = G.cuda().eval()
    size = cfg.crop_size
    renderer = SH.ViewRenderer(CS.bank("cuda"), size=S, views=c["V"], batch=1, near=c["near"], far=FAR)
    builder = SI.InputBuilder(S, S, size=size)
    args = (c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"])
    imgs, status = SH.shade_layouts(G, renderer, builder, *args, 2, draws=c["draws"].cuda(), rng=torch.Generator(device="cuda").manual_seed(5))
    _sync("shade_layouts")
    assert imgs.shape == (1, 2, size, size, 3) and imgs.dtype == torch.uint8 and imgs.is_cuda and status.tolist() == [0]
    assert not torch.equal(imgs[0, 0], imgs[0, 1]) and int(imgs.max()) > int(imgs.min())
    labels = renderer.labels.cpu()
    differ = labels[0] != w64["labels"][0]
    frac = float(differ.float().mean())
    print("class image: %.4f %% of the pixels differ from the float64 route (float32 host route: %.4f %%; cap 0.5 %%)" % (100 * frac, 100 * frac32))
    assert renderer.chosen.tolist() == w64["chosen"].tolist() and frac <= cap
    assert len(set(torch.unique(labels).tolist()) - {0}) >= 4
    # the images are the generator's on the builder's input of the renderer's planes
    total = builder.out.clone()
    again = SI.to_uint8(SI.colorize(G, builder(renderer.depth[0], labels=renderer.labels[0]), 2, torch.Generator(device="cuda").manual_seed(5)))
    assert torch.equal(again, imgs[0]) and torch.equal(builder.out, total)
    # the 41-channel input against the float64 route's
    width = int(SI.band_table(S, size)[1].shape[1])
    want = SI.build_input(w64["depth"][0], SI.masks_from_labels(w64["labels"][0]), size=size)[0]
    host32 = SI.build_input(w32["depth"][0], SI.masks_from_labels(w32["labels"][0]), size=size)[0]
    clean = _clean_outputs(differ | (w32["labels"][0] != w64["labels"][0]), S, size, width)
    assert float(clean.float().mean()) > 0.5
    got = total[0].cpu()
    cls_err = float((got[1:] - want[1:]).abs()[:, clean].max())
    d_err, d_host = float((got[0] - want[0]).abs()[clean].max()), float((host32[0] - want[0]).abs()[clean].max())
    print("input on %d clean pixels: class channels %.3e (bound 2e-6), depth channel %.3e (float32 host route %.3e, allowed four times that)"
          % (int(clean.sum()), cls_err, d_err, d_host))
    assert cls_err <= 2e-6 and d_err <= 4.0 * d_host


def test_second_call_and_graph_replay_give_the_same_bytes():
    _lib()
    SH = pkg("host.shade")
    c = CS.case("five_views")
    bnk = CS.bank("cuda")
    r = SH.ViewRenderer(bnk, size=c["S"], views=c["V"], batch=1, near=c["near"], far=FAR)
    args = (c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"])
    draws = c["draws"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r(*args, draws=draws)
        torch.cuda.synchronize()
        first = [t.clone() for t in (r.labels, r.depth, r.chosen, r.status, r.sums, r.faces_xyz)]
        r(*args, draws=draws)
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    _sync("two eager calls")
    second = (r.labels, r.depth, r.chosen, r.status, r.sums, r.faces_xyz)
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(_bits(first[1]), _bits(second[1]))
    assert torch.equal(first[4].view(torch.int64), r.sums.view(torch.int64)), "the reduction is fixed-order"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r(*args, draws=draws)
    for _ in range(2):
        for t in second:
            t.zero_()
        graph.replay()
        _sync("replay of the viewpoint render")
        assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(_bits(first[1]), _bits(second[1]))
    # other draws through the same graph: the draws are read on the device
    draws.copy_(torch.flip(draws, [1]))
    graph.replay()
    _sync("replay with other draws")
    assert not torch.equal(first[5], r.faces_xyz)


def test_a_room_without_an_acceptable_view_sets_status_and_raises_only_under_validate():
    _lib()
    SH, SI = pkg("host.shade"), pkg("host.spade_input")
    c = CS.case("one_view")
    bnk = CS.bank("cuda")
    args = (c["boxes"].cuda(), c["angles"].cuda(), c["objs"].cuda(), c["rows"])
    quiet = SH.ViewRenderer(bnk, size=c["S"], views=3, batch=1, min_mean_depth=50.0)
    labels, depth, chosen, status = quiet(*args, generator=torch.Generator(device="cuda").manual_seed(1))
    _sync("a room without an acceptable view")
    assert status.tolist() == [1] and chosen.tolist() == [0] and torch.equal(labels[0], quiet.labels_all[0])
    strict = SH.ViewRenderer(bnk, size=c["S"], views=3, batch=1, min_mean_depth=50.0, validate=True)
    with pytest.raises(ValueError, match="viewpoint"):
        strict(*args)
    fine = SH.ViewRenderer(bnk, size=c["S"], views=3, batch=1, validate=True)
    assert fine(*args)[3].tolist() == [0]
    with pytest.raises(ValueError):
        SH.shade_layouts(None, quiet, SI.InputBuilder(c["S"], c["S"], size=c["S"]), *args, 1, validate=True)
    _sync("validate")
