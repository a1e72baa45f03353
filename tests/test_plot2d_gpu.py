"""sln_layout_plot / sln_layout_footprint_counts (csrc/layout_plot.hip, host/plot2d.py) on the device: exact known answers, seeded random
layouts against the fp64 restatement outside the band of pixels within DELTA of a drawn edge line (tests/plot2d_cases.py), the
executed reference's pictures (tests/golden/plot2d.npz), the slice boundary of the layout axis and the argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import plot2d_cases as K
from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(c):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}


def _plot(c, N, **kw):
    d = _dev(c)
    return K.P().layout_plot(d["boxes"], d["angles"], d["room_of_row"], d["rank"], d["rgb"], size=N, room_id=d["room_id"], n_rooms=d["n_rooms"], **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# exact known answers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.known_cases()))
def test_known_answers_every_pixel(name):
    P = K.P()
    boxes, angles, rr, rank, rgb, want = K.known_inputs(name)
    winner, image = P.layout_plot(boxes.to(DEV), angles.to(DEV), rr.to(DEV), rank.to(DEV), rgb.to(DEV), size=K.KNOWN_N)
    assert torch.equal(winner[0, 0].cpu(), want), (name, winner[0, 0].cpu())
    assert torch.equal(image[0, 0].cpu(), K.palette_image(want, rgb))
    counts = P.layout_footprints(boxes.to(DEV), angles.to(DEV), rr.to(DEV), rank.to(DEV), size=K.KNOWN_N).cpu()
    for o in range(rank.numel()):                                          # one layout: a row's plane is where it covers, seen or hidden
        if int(rank[o]) >= 0:
            assert bool((counts[o][want == o] == 1).all()) and int(counts[o].max()) <= 1
        else:
            assert int(counts[o].abs().sum()) == 0


def test_sentinels_behind_the_outputs_are_untouched():
    """N = 17 (byte stores, partial tiles) and N = 8, N = 100 (dword stores): nothing is written behind either output"""
    L = pkg("_lib")
    c = _dev(K.random_case("two_rooms", 3))
    S, O, R = 3, c["boxes"].shape[1], c["n_rooms"]
    for N in (8, 17, 100):
        nw, ni = S * R * N * N, S * R * N * N * 3
        w = torch.full((nw + 64,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        im = torch.full((ni + 64,), 0x5a, dtype=torch.uint8, device=DEV)
        cnt = torch.full((O * N * N + 64,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        cnt[:O * N * N] = 0
        L.check(L.lib().sln_layout_plot(L.ptr(c["boxes"]), L.ptr(c["angles"]), L.ptr(c["room_of_row"]), L.ptr(c["room_id"]), L.ptr(c["rank"]),
                                        L.ptr(c["rgb"]), R, S, O, N, L.ptr(w), L.ptr(im), L.current_stream_ptr()), "sln_layout_plot")
        L.check(L.lib().sln_layout_footprint_counts(L.ptr(c["boxes"]), L.ptr(c["angles"]), L.ptr(c["room_of_row"]), L.ptr(c["rank"]), S, O, N, L.ptr(cnt),
                                                    L.current_stream_ptr()), "sln_layout_footprint_counts")
        assert bool((w[nw:] == 0x5a5a5a5a).all()) and bool((im[ni:] == 0x5a).all()) and bool((cnt[O * N * N:] == 0x5a5a5a5a).all()), N
        want_w, want_im = K.P().layout_plot(c["boxes"], c["angles"], c["room_of_row"], c["rank"], c["rgb"], size=N, room_id=c["room_id"], n_rooms=R)
        assert torch.equal(w[:nw].view_as(want_w), want_w) and torch.equal(im[:ni].view_as(want_im), want_im)


# ------------------------------------------------------------------------------------------------------------------------------
# random layouts against the fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", K.SIZES)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("kind", ["two_rooms", "long_room"])
def test_random_layouts_equal_the_fp64_restatement(kind, S, N):
    c = K.random_case(kind, S)
    want_w, want_im, excl = K.plot_reference(kind, S, N)
    share = excl.float().mean((2, 3))
    print("%s S %d N %d: excluded share per image %s" % (kind, S, N, share.flatten().tolist()))
    assert float(share.max()) <= 0.02
    winner, image = _plot(c, N)
    winner, image = winner.cpu(), image.cpu()
    bad = (winner != want_w) & ~excl
    print("    differing pixels outside the band: %d, inside: %d" % (int(bad.sum()), int(((winner != want_w) & excl).sum())))
    assert int(bad.sum()) == 0
    assert torch.equal(image[~excl], want_im[~excl])
    assert torch.equal(image, K.palette_image(winner, c["rgb"]))          # every pixel, nothing excluded
    only_w, none = _plot(c, N, want_rgb=False)
    none2, only_im = _plot(c, N, want_winner=False)
    assert none is None and none2 is None and torch.equal(only_w.cpu(), winner) and torch.equal(only_im.cpu(), image)


def test_fixture_rooms_equal_the_executed_reference():
    P = K.P()
    g = load_golden("plot2d")
    for name in bytes(g["rooms"]).decode().split(","):
        objs = torch.from_numpy(g[name + ":objs"])
        rank, rgb = P.plot_tables(objs, P.PLOT2D_CLASSES)
        O = objs.numel()
        boxes, angles = torch.from_numpy(g[name + ":boxes"]).to(DEV), torch.from_numpy(g[name + ":angles"]).to(DEV)
        _, image = P.layout_plot(boxes[None], angles[None], torch.full((O,), O - 1, dtype=torch.int32, device=DEV), rank.to(DEV), rgb.to(DEV), size=128)
        kept = g[name + ":kept"]
        assert kept.mean() >= 0.70
        diff = np.abs(image[0, 0].cpu().numpy().astype(np.int64) - g[name + ":image"].astype(np.int64)).max(-1)
        assert int((diff[kept] > 1).sum()) == 0, name
        # the drop-in: the reference's call shape returns the same picture
        again = P.plot2d(boxes, angles, objs, size=128)
        assert again.shape == (128, 128, 3) and torch.equal(again, image[0, 0])
        again = P.plot2d(boxes, angles.to(torch.int64), objs.tolist(), size=128)         # integer bins are converted
        assert torch.equal(again, image[0, 0])


def test_plot2d_with_the_references_own_example_call(tmp_path):
    """test.py:46-53 as it stands: lists of CPU tensors in, a file named as plt.savefig names it, the picture back on the CPU"""
    from PIL import Image
    P = K.P()
    boxes, rots, types = K.reference_example()
    image = P.plot2d(boxes, rots, types, str(tmp_path / "2D_rendered"), size=128)
    assert image.shape == (128, 128, 3) and image.dtype == torch.uint8 and image.device.type == "cpu"
    assert np.array_equal(np.asarray(Image.open(tmp_path / "2D_rendered.png").convert("RGB")), image.numpy())
    b, a, o = P._rows(boxes, torch.float32), P._rows(rots, torch.float32), torch.tensor(types)
    rank, rgb = P.plot_tables(o, P.PLOT2D_CLASSES)
    case = dict(boxes=b[None], angles=a[None], room_of_row=torch.full((6,), 5, dtype=torch.int32), rank=rank)
    _, want = P.layout_plot_torch(case["boxes"], case["angles"], case["room_of_row"], rank, rgb, size=128)
    excl = K.near_edges(case, 128).any(1)[0]
    assert float(excl.float().mean()) <= 0.02 and torch.equal(image[~excl], want[0, 0][~excl])
    colours = lambda im: {tuple(p) for p in im.reshape(-1, 3).tolist()}
    assert colours(image) == colours(want[0, 0]) and len(colours(image)) == 5   # the floor, a cabinet, a bed, a dresser, a desk (the window is not drawn)
    # CPU tensors (test_render_refine.py:294-295 passes .cpu().detach()) and cuda tensors give the same picture
    assert torch.equal(P.plot2d(b, a, o, size=128), image)
    on_dev = P.plot2d(b.to(DEV), a.to(DEV), o.to(DEV), size=128)
    assert on_dev.device.type == "cuda" and torch.equal(on_dev.cpu(), image)


def test_host_wrappers_refuse_what_the_kernels_cannot_take():
    P, L = K.P(), pkg("_lib")
    c = K.random_case("two_rooms", 1)
    d = _dev(c)
    args = lambda src: (src["boxes"], src["angles"], src["room_of_row"], src["rank"])
    with pytest.raises(L.SlnError):
        P.layout_plot(*args(c), c["rgb"], size=8)                              # everything on the CPU
    for name in ("angles", "room_of_row", "rank", "rgb"):
        mixed = dict(d, **{name: c[name]})
        with pytest.raises(L.SlnError):
            P.layout_plot(*args(mixed), mixed["rgb"], size=8)
    with pytest.raises(L.SlnError):
        P.layout_plot(*args(d), d["rgb"], size=8, room_id=c["room_id"], n_rooms=2)
    with pytest.raises(L.SlnError):
        P.layout_footprints(*args(d), size=8, counts=torch.zeros(d["boxes"].shape[1], 8, 8, dtype=torch.int32))
    # room_id without n_rooms: the number of rooms is read from the table
    w, _ = P.layout_plot(*args(d), d["rgb"], size=8, room_id=d["room_id"], want_rgb=False)
    w2, _ = P.layout_plot(*args(d), d["rgb"], size=8, want_rgb=False)
    assert w.shape == (1, 2, 8, 8) and torch.equal(w, w2)


# ------------------------------------------------------------------------------------------------------------------------------
# footprints
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 100])
def test_footprint_counts_equal_the_fp64_restatement(N):
    P = K.P()
    S = 257                                                                # two chunks of 128 layouts and a tail of one
    c = K.random_case("footprints", S)
    d = _dev(c)
    want, slack = K.footprint_reference("footprints", S, N)
    O = c["objs"].numel()
    hidden = [o for o in range(O) if int(c["rank"][o]) < 0]
    assert hidden and len(hidden) < O - 1
    counts = torch.zeros(O, N, N, dtype=torch.int32, device=DEV)
    counts[hidden] = 77                                                    # the planes of undrawn rows keep their sentinel
    out = P.layout_footprints(d["boxes"], d["angles"], d["room_of_row"], d["rank"], size=N, counts=counts)
    assert out is counts
    got = counts.cpu()
    assert bool((got[hidden] == 77).all())
    got[hidden] = 0
    diff = (got - want).abs()
    print("N %d: pixels in the band %d, differing there %d, elsewhere %d" % (N, int((slack > 0).sum()), int((diff > 0)[slack > 0].sum()),
                                                                             int((diff > 0)[slack == 0].sum())))
    assert int(want.sum()) > 0 and bool((diff <= slack).all())
    again = P.layout_footprints(d["boxes"], d["angles"], d["room_of_row"], d["rank"], size=N).cpu()
    assert torch.equal(again, got)                                         # bit-identical from run to run
    P.layout_footprints(d["boxes"], d["angles"], d["room_of_row"], d["rank"], size=N, counts=counts)
    twice = counts.cpu()
    twice[hidden] = 0
    assert torch.equal(twice, 2 * got)                                     # counts= accumulates


@pytest.mark.parametrize("N", [17, 100])
def test_footprints_agree_with_the_painter_for_a_one_object_room(N):
    P = K.P()
    c = K.random_case("one_object", 257)
    d = _dev(c)
    winner, _ = _plot(c, N, want_rgb=False)
    counts = P.layout_footprints(d["boxes"], d["angles"], d["room_of_row"], d["rank"], size=N)
    assert int(counts[0].sum()) > 0 and torch.equal(counts[0], (winner[:, 0] == 0).sum(0).to(torch.int32))


def test_footprints_from_words_is_the_plain_pipeline_on_its_samples():
    """one chunk == sample_layouts + layout_footprints on the same draws; chunks accumulate; undrawn planes stay 0"""
    from oracle import vae_ref
    P, S = K.P(), pkg("host.sampling")
    cfg = vae_ref.VaeConfig(embedding_dim=16, gconv_num_layers=2)
    model = pkg("host.Sg2ScVAE_model").Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict({k: v.clone() for k, v in vae_ref.init_state(cfg, seed=2).items()})
    model = model.cuda().eval()
    E = cfg.embedding_dim
    mean, cov = torch.zeros(E, dtype=torch.float64), torch.eye(E, dtype=torch.float64) * 0.25
    objs5 = ["bed", "desk", "door", "chair", "lamp"]
    rels5 = [("bed", "behind", "desk"), ("door", "left of", "bed"), ("chair", "left of", "desk"), ("lamp", "on", "desk")]
    got = S.footprints_from_words(model, objs5, rels5, mean, cov, num_iter=64, chunk=64, size=40, generator=torch.Generator().manual_seed(3))
    objs, triples, attrs = S.scene_graph_from_words(objs5, rels5, device=DEV)
    bp, ab, _ = S.sample_layouts(model, objs, triples, attrs, n_samples=64, mean=mean, cov=cov, generator=torch.Generator().manual_seed(3))
    rank, _ = P.plot_tables(objs, S.VALID_CLASSES)
    assert rank.tolist()[2] == -1 and rank.tolist()[5] == -1 and min(rank.tolist()[:2]) >= 0
    want = P.layout_footprints(bp, ab, torch.full((6,), 5, dtype=torch.int32, device=DEV), rank, size=40)
    assert got.shape == (6, 40, 40) and got.dtype == torch.int32 and torch.equal(got, want)
    assert int(got[2].abs().sum()) == 0 and int(got[5].abs().sum()) == 0 and int(got[0].sum()) > 0 and int(got.max()) <= 64
    g = torch.Generator().manual_seed(3)
    two = S.footprints_from_words(model, objs5, rels5, mean, cov, num_iter=96, chunk=64, size=40, generator=g)
    assert int(two.max()) <= 96 and bool((two >= got).all()) and int(two.sum()) > int(got.sum())


# ------------------------------------------------------------------------------------------------------------------------------
# the slice boundary of the layout axis, argument checks
# ------------------------------------------------------------------------------------------------------------------------------
def test_layouts_on_both_sides_of_the_slice_boundary():
    P = K.P()
    S, N = 65537, 8
    g = torch.Generator().manual_seed(5)
    lo = torch.rand(S, 1, 3, generator=g) * 0.5
    obj = torch.cat([lo, lo + 0.1 + 0.4 * torch.rand(S, 1, 3, generator=g)], -1)
    boxes = torch.cat([obj, torch.tensor([0, 0, 0, 1, 1, 1.0]).expand(S, 1, 6)], 1)
    angles = torch.cat([torch.randint(0, 24, (S, 1), generator=g).float(), torch.zeros(S, 1)], 1)
    objs = torch.tensor([K.cls("sofa"), 0])
    rank, rgb = P.plot_tables(objs, P.PLOT2D_CLASSES)
    rr = torch.tensor([1, 1], dtype=torch.int32)
    winner, image = P.layout_plot(boxes.to(DEV), angles.to(DEV), rr.to(DEV), rank.to(DEV), rgb.to(DEV), size=N)
    pick = [0, 65534, 65535, 65536]
    case = dict(boxes=boxes[pick], angles=angles[pick], room_of_row=rr, rank=rank)
    want_w, want_im = P.layout_plot_torch(boxes[pick], angles[pick], rr, rank, rgb, size=N)
    excl = K.near_edges(case, N).any(1)[:, None]
    assert float(excl.float().mean()) <= 0.02
    got_w, got_im = winner[pick].cpu(), image[pick].cpu()
    assert torch.equal(got_w[~excl], want_w[~excl]) and torch.equal(got_im[~excl], want_im[~excl])
    assert len({int((want_w[i] >= 0).sum()) for i in range(4)}) > 1 and int((want_w >= 0).sum()) > 0      # (the four layouts differ)


def test_bad_arguments_are_refused_before_any_launch():
    L = pkg("_lib")
    c = _dev(K.random_case("two_rooms", 1))
    O, R = c["boxes"].shape[1], c["n_rooms"]
    w = torch.full((R * 8 * 8,), 7, dtype=torch.int32, device=DEV)
    im = torch.full((R * 8 * 8 * 3,), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.full((O * 8 * 8,), 7, dtype=torch.int32, device=DEV)
    p, st = L.ptr, L.current_stream_ptr()
    plot = lambda boxes, N, wp, ip: L.lib().sln_layout_plot(boxes, p(c["angles"]), p(c["room_of_row"]), p(c["room_id"]), p(c["rank"]), p(c["rgb"]),
                                                            R, 1, O, N, wp, ip, st)
    foot = lambda boxes, N, cp: L.lib().sln_layout_footprint_counts(boxes, p(c["angles"]), p(c["room_of_row"]), p(c["rank"]), 1, O, N, cp, st)
    assert plot(p(c["boxes"]), 0, p(w), p(im)) == -1 and plot(p(c["boxes"]), 1025, p(w), p(im)) == -1
    assert plot(None, 8, p(w), p(im)) == -1 and plot(p(c["boxes"]), 8, None, None) == -1
    assert foot(p(c["boxes"]), 0, p(cnt)) == -1 and foot(p(c["boxes"]), 1025, p(cnt)) == -1
    assert foot(None, 8, p(cnt)) == -1 and foot(p(c["boxes"]), 8, None) == -1
    torch.cuda.synchronize()
    assert bool((w == 7).all()) and bool((im == 7).all()) and bool((cnt == 7).all())
    assert plot(p(c["boxes"]), 8, p(w), None) == 0 and plot(p(c["boxes"]), 8, None, p(im)) == 0 and foot(p(c["boxes"]), 8, p(cnt)) == 0
    P = K.P()
    with pytest.raises(ValueError):
        P.layout_plot(c["boxes"], c["angles"], c["room_of_row"], c["rank"], c["rgb"], size=0)
    with pytest.raises(ValueError):
        P.layout_footprints(c["boxes"], c["angles"], c["room_of_row"], c["rank"], size=1025)
