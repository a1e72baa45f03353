"""Viewpoint render, host side (host/shade.py; CPU-only): the torch restatements against what the reference's own statements computed
(tests/golden/shade_view.npz, tools/gen_golden_shade_view.py), the stated camera convention, the CPU route on a golden room, and the
argument checks of ``sln_view_place_project`` (which run before anything is launched, so they need no device)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import shade_view_cases as CS
from conftest import ROOT, load_golden, pkg

T = torch.from_numpy


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_shade_view", os.path.join(ROOT, "tools", "gen_golden_shade_view.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_regenerates_bit_for_bit(tmp_path):
    tool = _tool()
    if not os.path.isdir(tool.REF):
        pytest.skip("the reference tree is not on this machine")
    path = str(tmp_path / "shade_view.npz")
    tool.main(path)
    assert open(path, "rb").read() == open(os.path.join(ROOT, "tests", "golden", "shade_view.npz"), "rb").read()


def test_placement_equals_the_reference_bit_for_bit():
    SH = pkg("host.shade")
    g = load_golden("shade_view")
    models = T(g["row_model"]).clamp(min=0)
    pl = SH.shade_placement(T(g["boxes"]), T(g["angles"]), models, T(g["room_row"]), T(g["model_bbox"]))
    obj = g["row_model"] >= 0
    assert obj.sum() >= 30
    for key, want in (("A", g["A"]), ("tr", g["tr"]), ("center", g["center"]), ("scaled_size", g["scaled_size"]), ("boxes", g["restored"])):
        got = pl[key].numpy()
        assert got.dtype == np.float64 and np.array_equal(got[obj], want[obj]), key
    # the fixture holds what it is there for: heights snapped from both signs, the threshold from both sides, a room row with an origin
    y0 = g["boxes"][:, 1] * (g["boxes"][g["room_row"], 4] - g["boxes"][g["room_row"], 1])
    snapped = obj & (g["restored"][:, 1] == 0) & (g["boxes"][:, 1] != 0)
    assert (snapped & (y0 > 0)).any() and (snapped & (y0 < 0)).any() and (obj & (y0 > 0.02) & (y0 < 0.0202)).any() and (g["boxes"][g["room_row"], 0] > 0).any()
    assert (np.abs(y0[snapped]) <= 0.02).all() and not (obj & ~snapped & (np.abs(y0) <= 0.02) & (g["boxes"][:, 1] != 0)).any()
    # the model rests on the bottom of its box (:228), which the refinement's placement does not do
    lo_y = g["center"][obj, 1] - g["scaled_size"][obj, 1] / 2
    assert np.abs(lo_y - g["restored"][obj, 1]).max() < 1e-12
    # float32: the same statements, to float32's precision
    pl32 = SH.shade_placement(T(g["boxes"]).float(), T(g["angles"]).float(), models, T(g["room_row"]), T(g["model_bbox"]).float())
    assert pl32["A"].dtype == torch.float32 and float((pl32["tr"].double() - pl["tr"])[T(obj)].abs().max()) < 1e-5


def test_viewpoint_equals_the_reference_bit_for_bit_and_the_list_is_the_references():
    SH = pkg("host.shade")
    g = load_golden("shade_view")
    room = g["boxes"][np.unique(g["room_row"])]
    ext = T(room[:, 3:] - room[:, :3])[:, None, :].expand(-1, 5, 3)
    cam, canonical, plane = SH.shade_viewpoint(ext, T(g["draws"][..., 0]), T(g["draws"][..., 1]))
    assert np.array_equal(cam.numpy(), g["cam_coord"]) and np.array_equal(canonical.numpy(), g["canonical_angle"])
    assert np.array_equal(plane.numpy(), g["plane_angle"])
    assert tuple(bytes(g["not_imported"]).decode().split("\n")) == SH.NOT_IMPORTED
    assert SH.N_SAMPLE == g["draws"].shape[1] == 5


def test_acceptance_choice_equals_the_reference_in_every_case():
    SH = pkg("host.shade")
    g = load_golden("shade_view")
    names = bytes(g["accept_names"]).decode().split("\n")
    z = T(g["accept_z"])                                            # [cases, 5, h, w] float64; every sum exact in any order
    below = z < SH.MEAN_BELOW
    sums, counts = torch.where(below, z, torch.zeros_like(z)).sum(dim=(2, 3)), below.sum(dim=(2, 3))
    seen = set()
    for i, name in enumerate(names):
        thr = SH.MIN_MEAN_DEPTH if np.isnan(g["accept_threshold"][i]) else float(g["accept_threshold"][i])
        chosen, status = SH.choose_view(sums[i:i + 1], counts[i:i + 1], thr)
        want = int(g["accept_chosen"][i])
        assert (int(status[0]), int(chosen[0])) == ((1, 0) if want < 0 else (0, want)), name
        seen.add(want)
        if "at_threshold" in name:                                  # the strict > : a view whose mean IS the threshold is not accepted
            mean = sums[i] / counts[i]
            assert bool((mean == thr).any()) and not bool(((mean == thr) & (torch.arange(5) == want)).any())
    assert {-1, 0, 2, 4} <= seen
    # a view without an entry below 1e5 is not accepted (the reference divides by zero there)
    chosen, status = SH.choose_view(torch.tensor([[0.0, 5.0]], dtype=torch.float64), torch.tensor([[0, 4]]))
    assert chosen.tolist() == [1] and status.tolist() == [0]
    assert SH.choose_view(torch.zeros(1, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int64))[1].tolist() == [1]


def _project(K, R, t, p, S):
    cam = R @ p + t
    u = K @ (cam / cam[2])
    return float(u[0]), float(S - u[1]), float(cam[2])


def test_the_stated_convention_is_sane_on_the_golden_rooms():
    """The viewpoint looks down by canonical_angle (about 54 degrees) from 0.4 m outside the room, with a half angle of atan(1/2): plain
    trigonometry says where the back wall's centre is inside the picture - at a depression atan(0.4 h / (z + 0.4)) of at least
    canonical_angle - atan(1/2) - and the golden rooms are shallow enough for that.  There it must project inside the image, in front
    of the camera; and a camera to the right of the room's middle looks left."""
    SH = pkg("host.shade")
    g = load_golden("shade_view")
    room = g["boxes"][np.unique(g["room_row"])]
    ext = room[:, 3:] - room[:, :3]
    S = 64
    K, R, t = SH.shade_camera(T(ext)[:, None, :].expand(-1, 5, 3), T(g["draws"][..., 0]), T(g["draws"][..., 1]), S)
    checked = 0
    for r in range(len(ext)):
        for v in range(5):
            Rm, tv = R[r, v].numpy(), t[r, v].numpy()
            assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(Rm) - 1) < 1e-12
            assert np.allclose(-Rm.T @ tv, g["cam_coord"][r, v], atol=1e-12)
            depression = np.arctan(0.4 * ext[r, 1] / (ext[r, 2] + 0.4))
            assert depression > g["canonical_angle"][r, v] - np.arctan(0.5) + 0.02, "a golden room too deep for this check"
            x, y, z = _project(K[r, v].numpy(), Rm, tv, np.array([ext[r, 0] / 2, ext[r, 1] / 2, 0.0]), S)
            assert z > ext[r, 2] * 0.5 and 0 < x < S and 0 < y < S, (r, v, x, y, z)
            # +y of the image is up: the floor's back edge lies below the back wall's centre
            assert _project(K[r, v].numpy(), Rm, tv, np.array([ext[r, 0] / 2, 0.0, 0.0]), S)[1] < y
            look = Rm[2]                                              # the renderer's +z (the viewing direction) in room coordinates
            pos = 0.2 + 0.6 * g["draws"][r, v, 0]
            if abs(pos - 0.5) > 0.02:
                assert (look[0] < 0) == (pos > 0.5) and look[2] < 0 and look[1] < 0, (r, v, look)
                checked += 1
    assert checked >= 20


def test_procedural_shell_on_the_device_route_is_place_shell_bit_for_bit():
    SH, RF = pkg("host.shade"), pkg("host.refine")
    bnk = CS.bank("cpu")
    tables = SH.BankTables.of(bnk, "cpu")
    ext = torch.tensor([[4.0, 2.7, 5.0], [3.1415927, 2.4000001, 2.0999999], [2.5, 3.2, 4.7]], dtype=torch.float32)
    got = SH.procedural_shell(tables, ext)
    for r in range(3):
        assert torch.equal(got[r], RF.place_shell(bnk, ext[r].tolist())), r
    assert tables.Fs == sum(f.shape[0] for _, _, f in RF.shell_topology(bnk)) and int(tables.shell_f_host.max()) == tables.Vs - 1
    assert sorted(set(tables.shell_label[:tables.Fs].tolist())) == [1, 2, 22]


def test_a_bank_with_shell_meshes_takes_place_shell_vertices():
    from oracle import raster_ref
    SH, RF = pkg("host.shade"), pkg("host.refine")
    bnk = CS.shell_bank("cpu")
    tables = SH.BankTables.of(bnk, "cpu")
    topo = RF.shell_topology(bnk)
    assert tables.shell_unit is None and tables.Fs == sum(f.shape[0] for _, _, f in topo) and tables.Vs == sum(nv for _, nv, _ in topo)
    assert tables.shell_label[:tables.Fs].tolist() == [1] * 16 + [2] * 12 + [22] * 12
    with pytest.raises(pkg("_lib").SlnError, match="bind_shell"):
        SH.procedural_shell(tables, torch.ones(1, 3))
    c = CS.case("five_views")
    c["objs"] = torch.where((c["objs"] == 1) | (c["objs"] == 3), c["objs"], torch.zeros_like(c["objs"]))
    ext = c["boxes"][-1, 3:].tolist()
    shell_v = RF.place_shell(bnk, ext)[None]
    got = SH.views_torch(bnk, c["boxes"], c["angles"], c["objs"], c["rows"], c["draws"], raster_ref.nmr_forward, size=c["S"], views=c["V"], shell_v=shell_v)
    F = got["faces_xyz"].shape[1]
    assert F == max(c["rows"]) * tables.Fm + tables.Fs and got["status"].tolist() == [0]
    seen = set(torch.unique(got["labels_all"]).tolist())
    assert 2 in seen and seen <= {0, 1, 2, 22, 1 + SH.NYU40.index("bed"), 1 + SH.NYU40.index("desk")}


def test_views_torch_on_a_golden_room_chooses_the_recorded_view():
    from oracle import raster_ref
    SH, RF, syn = pkg("host.shade"), pkg("host.refine"), pkg("host.synthetic")
    g = load_golden("shade_view")
    tool = _tool()
    bnk = tool.view_bank(RF, syn, g["view_sizes"])
    args = (bnk, T(g["view_boxes"]).double(), T(g["view_angles"]).double(), T(g["view_objs"]).long(), [3], T(g["view_draws"]), raster_ref.nmr_forward)
    for thr, want in zip(g["view_threshold"].tolist(), g["view_chosen"].tolist()):
        got = SH.views_torch(*args, size=int(g["view_S"][0]), vocab=tool.VOCAB, min_mean_depth=thr)
        assert got["chosen"].tolist() == [want] and got["status"].tolist() == [0]
        np.testing.assert_allclose((got["sums"] / got["counts"]).numpy(), g["view_means"], rtol=1e-9)
        assert torch.equal(got["labels"][0], got["labels_all"][want]) and torch.equal(got["depth"][0], got["depth_all"][want])
    cab, bed = 1 + SH.NYU40.index("cabinet"), 1 + SH.NYU40.index("bed")
    assert set(torch.unique(got["labels_all"]).tolist()) <= {0, 1, 2, 22, cab, bed} and bool((got["labels_all"][0] == cab).any())
    assert float(got["depth_all"].max()) == 1e10 or bool((got["labels_all"] > 0).all())
    none = SH.views_torch(*args, size=int(g["view_S"][0]), vocab=tool.VOCAB, min_mean_depth=50.0)
    assert none["status"].tolist() == [1] and none["chosen"].tolist() == [0]


def test_fp32_restatement_stays_inside_the_figure_the_kernel_is_allowed_four_times_of():
    import test_shade_view_gpu as G
    SH = pkg("host.shade")
    bnk = CS.bank("cpu")
    worst = 0.0
    for name, *_ in CS.CASES:
        c = CS.case(name)
        want, got = CS.torch_route(SH, bnk, c, torch.float64), CS.torch_route(SH, bnk, c, torch.float32)
        err, flips = CS.face_error(got["faces_xyz"], want["faces_xyz"])
        assert flips == 0 and torch.equal(got["face_label"], want["face_label"]), name
        print("%s: fp32 torch against fp64, largest |d| / max(1, |want|) = %.3e" % (name, err))
        worst = max(worst, err)
        fx = want["faces_xyz"]
        live = ~(fx == 0).all(-1).all(-1)
        if name == "every_face_culled":
            assert not bool(live.any())
        elif name == "no_visible_row":
            assert bool((want["rt"]["row_model"] < 0).all()) and bool(live.any())          # the shell alone
        else:
            assert bool((want["rt"]["row_model"] >= 0).any()) and bool(live[:, :fx.shape[1] - 360].any())
    print("largest: %.3e (FP32_TORCH_ERR %.3e)" % (worst, G.FP32_TORCH_ERR))
    assert worst <= G.FP32_TORCH_ERR <= 2.0 * worst


def test_save_color_has_the_references_call_shape(tmp_path):
    SH = pkg("host.shade")
    data = torch.linspace(-1, 1, 3 * 8 * 8).reshape(1, 3, 8, 8)
    folder = str(tmp_path / "images")
    path = SH.save_color(data, folder_name=folder, prefix="room_000")
    assert os.path.isdir(folder)
    if path is not None:                                            # (without PIL the writer warns and writes nothing)
        from PIL import Image
        assert path.endswith("room_000_color.png")
        got = np.asarray(Image.open(path))
        assert got.shape == (8, 8, 3) and np.array_equal(got, ((data[0].numpy() + 1.0) / 2.0).transpose(1, 2, 0).__mul__(255.0).astype(np.uint8))


def _descriptor(SH, L, tables, R=1, V=1, N=2):
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    rt = dict(A=f32(R, N, 3, 3), tr=f32(R, N, 3), row_model=torch.full((R, N), -1, dtype=torch.int32), row_label=torch.zeros(R, N, dtype=torch.uint8))
    F = N * tables.Fm + tables.Fs
    return rt, f32(R, tables.Vs, 3), f32(R, V, 3, 3), f32(R, V, 3, 3), f32(R, V, 3), f32(R * V, F, 3, 3), torch.zeros(R, F, dtype=torch.uint8)


def test_argument_checks_refuse_tables_that_point_past_the_bank():
    """every refusal returns before a launch: host tensors stand in for the device buffers, none is read"""
    import copy
    SH, L = pkg("host.shade"), pkg("_lib")
    base = SH.BankTables(CS.bank("cpu"), "cpu")
    assert base.M == 6 and base.Fm == 108 and base.voff_host[-1] == base.Vtot and base.foff_host[-1] == base.Ftot

    def refused(edit, **shape):
        tb = copy.copy(base)
        tb.voff_host, tb.foff_host, tb.shell_f_host = base.voff_host.copy(), base.foff_host.copy(), base.shell_f_host.copy()
        edit(tb)
        rt, shell_v, K, Rm, t, fx, fl = _descriptor(SH, L, tb, **shape)
        with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
            SH.place_project(tb, rt, shell_v, K, Rm, t, 64, 0.1, fx, fl)

    def past_the_vertices(tb): tb.voff_host[-1] += 1
    def past_the_faces(tb): tb.foff_host[-1] += 1
    def decreasing(tb): tb.voff_host[2] = tb.voff_host[1] - 1
    def not_from_zero(tb): tb.foff_host[0] = 1
    def more_faces_than_slots(tb): tb.Fm = 107
    def shell_corner_past_its_vertices(tb): tb.shell_f_host[5, 1] = tb.Vs
    def negative_shell_corner(tb): tb.shell_f_host[0, 0] = -1
    def smaller_bank(tb): tb.Vtot -= 1
    for edit in (past_the_vertices, past_the_faces, decreasing, not_from_zero, more_faces_than_slots, shell_corner_past_its_vertices,
                 negative_shell_corner, smaller_bank):
        refused(edit)
    refused(lambda tb: None, R=257, V=256)                          # more views than one launch's grid takes
    with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
        SH.compose(torch.zeros(3, 8, 8, dtype=torch.int32), torch.zeros(3, 8, 8), torch.zeros(1, 4, dtype=torch.uint8), 2, torch.zeros(999, dtype=torch.int64),
                   torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(3, 8, 8), torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int64))
    assert L.lib().sln_view_compose_workspace_bytes(0) < 0 and L.lib().sln_view_compose_workspace_bytes(5) == 5 * 128 * 16
