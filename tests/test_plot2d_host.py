"""Top-down layout pictures and footprint heat maps (host/plot2d.py) on the CPU: the row tables, the torch restatements of both kernels
against the executed reference (tests/golden/plot2d.npz, tools/gen_golden_plot2d.py), a brute-force loop and the exact known answers;
the conditions the GPU tests rely on (share of excluded pixels of the seeded random cases)."""
import numpy as np
import pytest
import torch

import plot2d_cases as K
from conftest import load_golden, pkg


def _rooms():
    g = load_golden("plot2d")
    return g, bytes(g["rooms"]).decode().split(",")


def _room_inputs(g, name):
    P = K.P()
    objs = torch.from_numpy(g[name + ":objs"])
    rank, rgb = P.plot_tables(objs, P.PLOT2D_CLASSES)
    O = objs.numel()
    return objs, torch.from_numpy(g[name + ":boxes"])[None], torch.from_numpy(g[name + ":angles"])[None], torch.full((O,), O - 1, dtype=torch.int32), rank, rgb


def test_plot_tables_equal_the_references_colours_and_order():
    P = K.P()
    g, rooms = _rooms()
    assert len(rooms) >= 3
    for name in rooms:
        objs, _, _, _, rank, rgb = _room_inputs(g, name)
        # order / order_rank are the output of the reference's own sorted(zip(current_types, iter_idx)) (:118-120), as recorded
        order = g[name + ":order"].tolist()
        drawn = [o for o in range(objs.numel()) if int(rank[o]) >= 0]
        assert sorted(drawn) == sorted(order)                                  # the rows the reference keeps (:86)
        assert [int(rank[o]) for o in order] == g[name + ":order_rank"].tolist()
        assert sorted(drawn, key=lambda o: (int(rank[o]), o)) == order
        got = K.palette_image(torch.tensor(order, dtype=torch.int32), rgb).numpy()
        assert np.array_equal(got, g[name + ":colors"]), name
        assert tuple(g[name + ":floor"].tolist()) == P.FLOOR_RGB
    assert rank.dtype == torch.int32 and rgb.dtype == torch.uint32
    assert len(P.PLOT2D_CLASSES) == 32 and set(P.DO_NOT_VIS) < set(P.PLOT2D_CLASSES) | {"ceiling"}


def test_plot_tables_raise_for_a_class_the_reference_could_not_index():
    P = K.P()
    names = ["__room__", "wall", "piano"]
    rank, _ = P.plot_tables(torch.tensor([1, 0]), names)                  # do_not_vis and room rows are never looked up
    assert rank.tolist() == [-1, -1]
    with pytest.raises(ValueError):
        P.plot_tables(torch.tensor([2, 0]), names)


def test_restatement_equals_the_executed_reference():
    """rings = the captured patch vertices (y = 1 - z) to 1e-6, the same draw order, the Agg image on every kept pixel"""
    P = K.P()
    g, rooms = _rooms()
    for name in rooms:
        objs, boxes, angles, rr, rank, rgb = _room_inputs(g, name)
        order = g[name + ":order"].tolist()
        ring = P.rings_torch(boxes, angles, rr, torch.float64)[0]
        got = torch.stack([ring[order, :, 0], 1.0 - ring[order, :, 1]], -1).numpy()
        assert np.abs(got - g[name + ":verts"]).max() <= 1e-6, name
        winner, image = P.layout_plot_torch(boxes, angles, rr, rank, rgb, size=128)
        kept = g[name + ":kept"]
        assert kept.mean() >= 0.70, name
        diff = np.abs(image[0, 0].numpy().astype(np.int64) - g[name + ":image"].astype(np.int64)).max(-1)
        assert int((diff[kept] > 1).sum()) == 0, name
        assert torch.equal(image, K.palette_image(winner, rgb))
        # the painter is a max over (rank, row): the last patch of the draw order that covers a pixel
        top = torch.full((128, 128), -1, dtype=torch.int32)
        for o in order:
            top[P.coverage_torch(ring[o], 128)] = o
        assert torch.equal(winner[0, 0], top), name


def test_plot2d_takes_the_references_data_format_and_never_a_host_pointer():
    """test.py:46-53: a list of [6] CPU tensors, a list of 0-d tensors, a list of ints.  The rows are stacked; the picture is drawn on
    the device (no device: SlnError, never a launch on host memory); layout_plot / layout_footprints refuse CPU tensors"""
    P, L = K.P(), pkg("_lib")
    boxes, rots, types = K.reference_example()
    b, a, o = P._rows(boxes, torch.float32), P._rows(rots, torch.float32), P._rows(types, torch.int64)
    assert b.shape == (6, 6) and a.shape == (6,) and o.tolist() == types and float(a[1]) == rots[1].item()
    rank, rgb = P.plot_tables(o, P.PLOT2D_CLASSES)
    assert rank.tolist() == [-1, P.NYU_CLASS_ORDER.index("cabinet"), 39, P.NYU_CLASS_ORDER.index("dresser"), P.NYU_CLASS_ORDER.index("desk"), -1]
    rr = torch.full((6,), 5, dtype=torch.int32)
    for call in (lambda: P.layout_plot(b[None], a[None], rr, rank, rgb, size=16), lambda: P.layout_footprints(b[None], a[None], rr, rank, size=16)):
        with pytest.raises(L.SlnError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        P.plot2d(boxes[:5], rots, types)
    if not torch.cuda.is_available():
        with pytest.raises(L.SlnError, match="no CPU fallback"):
            P.plot2d(boxes, rots, types, None)
        return
    image = P.plot2d(boxes, rots, types, None, size=64)                       # (the whole suite on the GPU machine: tests/test_plot2d_gpu.py checks it)
    assert image.shape == (64, 64, 3) and image.device.type == "cpu"


def test_save_png_appends_the_extension_savefig_would(tmp_path):
    from PIL import Image
    P = K.P()
    img = torch.arange(5 * 7 * 3, dtype=torch.uint8).reshape(5, 7, 3)
    assert P.save_png(img, str(tmp_path / "2D_rendered")) == str(tmp_path / "2D_rendered.png")        # plt.savefig("2D_rendered") (:140)
    assert P.save_png(img, tmp_path / "named.png") == str(tmp_path / "named.png")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["2D_rendered.png", "named.png"]
    for n in ("2D_rendered.png", "named.png"):
        assert np.array_equal(np.asarray(Image.open(tmp_path / n).convert("RGB")), img.numpy())


def test_footprints_restatement_equals_a_brute_force_loop():
    P = K.P()
    c = K.random_case("footprints", 3)
    N = 9
    got = P.layout_footprints_torch(c["boxes"], c["angles"], c["room_of_row"], c["rank"], size=N)
    ring = P.rings_torch(c["boxes"], c["angles"], c["room_of_row"], torch.float64).numpy()
    want = np.zeros((ring.shape[1], N, N), np.int32)
    for s in range(3):
        for o in range(ring.shape[1]):
            if int(c["rank"][o]) < 0:
                continue
            q = ring[s, o]
            for r in range(N):
                for col in range(N):
                    x, z = (col + 0.5) / N, (r + 0.5) / N
                    e = [(q[(k + 1) % 4][0] - q[k][0]) * (z - q[k][1]) - (q[(k + 1) % 4][1] - q[k][1]) * (x - q[k][0]) for k in range(4)]
                    want[o, r, col] += all(v >= 0 for v in e) or all(v <= 0 for v in e)
    assert want.sum() > 0 and np.array_equal(got.numpy(), want)
    again = P.layout_footprints_torch(c["boxes"], c["angles"], c["room_of_row"], c["rank"], size=N, counts=got.clone())
    assert torch.equal(again, 2 * got)


@pytest.mark.parametrize("name", sorted(K.known_cases()))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_known_answers_through_the_restatement(name, dtype):
    P = K.P()
    boxes, angles, rr, rank, rgb, want = K.known_inputs(name)
    winner, image = P.layout_plot_torch(boxes, angles, rr, rank, rgb, size=K.KNOWN_N, dtype=dtype)
    assert torch.equal(winner[0, 0], want), (name, winner[0, 0])
    assert torch.equal(image[0, 0], K.palette_image(want, rgb))
    counts = P.layout_footprints_torch(boxes, angles, rr, rank, size=K.KNOWN_N, dtype=dtype)
    if name in ("edge_on_centres", "swapped_x"):
        assert torch.equal(counts[0], (want == 0).to(torch.int32)) and int(counts[0].sum()) == 5 * 4
    if name in ("zero_width", "nothing_drawn"):
        assert int((want >= 0).sum()) == 0


def test_known_answers_say_what_the_issue_says():
    w = {n: K.known_inputs(n)[5] for n in K.known_cases()}
    assert torch.equal(w["edge_on_centres"], w["swapped_x"]) and bool((w["edge_on_centres"][2:6, 1:6] == 0).all())
    assert bool((w["nan"] != 0).all()) and int((w["nan"] == 1).sum()) == 16
    assert int(w["same_class"][3, 3]) == 1 and int(w["same_class"][1, 1]) == 0                    # the higher row wins the overlap
    for n, (bed, tv, chair) in (("order_a", (0, 1, 2)), ("order_b", (2, 1, 0))):
        assert int(w[n][2, 2]) == bed and int(w[n][2, 5]) == bed and int(w[n][1, 5]) == tv and int(w[n][1, 1]) == chair, n


@pytest.mark.parametrize("kind", ["two_rooms", "long_room"])
def test_random_cases_exclude_at_most_two_percent_of_an_image(kind):
    """the condition of the GPU comparison, on the fp64 reference alone"""
    for S in (1, 3):
        c = K.random_case(kind, S)
        assert set(c["angles"].flatten().tolist()) <= set(range(24))
        for N in K.SIZES:
            w, _, excl = K.plot_reference(kind, S, N)
            assert float(excl.float().mean((2, 3)).max()) <= 0.02, (kind, S, N)
            assert int((w >= 0).sum()) > 0
    c = K.random_case("two_rooms", 3)
    assert torch.bincount(c["room_id"].long()).tolist() == [4, 11]
    assert len(set(K.random_case("two_rooms", 3)["angles"].flatten().tolist())) >= 12
    long = K.random_case("long_room", 3)                                  # stage cap + 1 object rows: the last one is drawn and seen
    assert long["objs"].numel() == K.P().STAGE_ROWS + 2 and int(long["rank"][K.P().STAGE_ROWS]) >= 0
    assert all(int((K.plot_reference("long_room", 3, 128)[0][s] == K.P().STAGE_ROWS).sum()) > 0 for s in range(3))


def test_ctypes_table_lists_the_new_symbols():
    L = pkg("_lib")
    assert {"sln_layout_plot", "sln_layout_footprint_counts"} <= set(L.SIGNATURES)
    assert len(L.SIGNATURES["sln_layout_plot"][1]) == 13 and len(L.SIGNATURES["sln_layout_footprint_counts"][1]) == 9
