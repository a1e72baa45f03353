"""3-D drawing, host side (host/draw3d.py; CPU-only): the module's constants against what the reference's own statements computed
(tests/golden/draw3d.npz, tools/gen_golden_draw3d.py), the shading model in torch ops against closed forms on hand-made scenes, the
float32 restatement's own error on the room cases (the figure the kernel is allowed four times of), and the argument checks of
``sln_draw3d`` (which run before anything is launched, so they need no device)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import draw3d_cases as DC
from conftest import ROOT, load_golden, pkg


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_draw3d", os.path.join(ROOT, "tools", "gen_golden_draw3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_regenerates_bit_for_bit(tmp_path):
    tool = _tool()
    if not os.path.isdir(tool.REF):
        pytest.skip("the reference tree is not on this machine")
    path = str(tmp_path / "draw3d.npz")
    tool.main(path)
    assert open(path, "rb").read() == open(os.path.join(ROOT, "tests", "golden", "draw3d.npz"), "rb").read()


def test_constants_light_position_and_file_names_are_the_references():
    D = pkg("host.draw3d")
    g = load_golden("draw3d")
    assert g["resolution"].tolist() == [D.RESOLUTION, D.RESOLUTION, D.RESOLUTION_PERCENTAGE] == [1024, 1024, 25]
    assert set(g["light_energy"].tolist()) == {D.LIGHT_ENERGY} and set(g["light_size"].tolist()) == {D.LIGHT_SIZE}
    assert D.LIGHT_AT == (0.5, 0.9, 0.5) and D.N_PRED == 4
    ext = torch.from_numpy(g["extents"])
    assert ext.shape == (4, 3) and np.array_equal(D.light_position(ext).numpy(), g["light_xyz"])
    assert np.array_equal(D.light_position(g["extents"][2].tolist()).numpy(), g["light_xyz"][2])
    assert D.light_position(ext.float()).dtype == torch.float32
    # the geometry statements are the semantic render's: placement, shell, viewpoint loop
    assert g["same_geometry"].dtype == np.bool_ and g["same_geometry"].tolist() == [True, True, True]
    names = bytes(g["names"]).decode().split("\n")
    assert D.picture_names(_tool().two_rooms()) == names and len(names) == 8 and names[5] == "bedroom_17_pred_01_3d.png"
    assert D.percentage_k(D.RESOLUTION, D.RESOLUTION_PERCENTAGE) == 4
    for size, pct in ((1024, 30), (10, 25), (64, 5), (64, 0)):
        with pytest.raises(ValueError):
            D.percentage_k(size, pct)


def test_srgb_table_and_albedo():
    D, SP = pkg("host.draw3d"), pkg("host.scene_pictures")
    v = np.arange(256, dtype=np.float64) / 255.0
    want = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    got = D.srgb_to_linear(torch.from_numpy(v))
    assert np.allclose(got.numpy(), want, rtol=1e-14, atol=0) and got[0] == 0 and abs(float(got[255]) - 1.0) < 1e-15
    back = D.linear_to_srgb(got) * 255.0
    assert float((back - torch.arange(256).double()).abs().max()) < 1e-9, "the two transfer functions are each other's inverse on the bytes"
    assert bool((np.diff(want) > 0).all())
    alb = D.albedo_table()
    assert alb.shape == (41, 3) and alb.dtype == torch.float32 and len(SP.CLASS_COLORS) == 41 and alb[0].tolist() == [0.0, 0.0, 0.0]
    for i in (1, 2, 22, 40):
        for ch in range(3):
            assert float(alb[i, ch]) == float(np.float32(want[SP.CLASS_COLORS[i][ch]]))
    assert len(set(map(tuple, alb.tolist()))) >= 30


def _sample_point(S, yi, xi, z):
    """the hit point of raster sample (yi, xi) at depth z under the module's K"""
    return np.array([(2 * xi + 1 - S) / S / 2.0, -(2 * yi + 1 - S) / S / 2.0, 1.0]) * z


def test_floor_under_the_lamp_has_the_analytic_irradiance():
    D = pkg("host.draw3d")
    op, w = DC.operands("floor"), DC.want("floor")
    S, lamp = op["S"], np.asarray(DC.LAMP)
    alb = D.albedo_table().double()[2].numpy()
    assert int(w["hit"].sum()) == 484 and bool(w["visible"].all()) and not bool(w["unsafe"].any())
    for yi, xi in ((5, 5), (16, 16), (26, 7), (12, 20), (15, 17)):
        assert bool(w["hit"][0, yi, xi])
        p = _sample_point(S, yi, xi, DC.FLOOR_Z)
        l = lamp - p
        E = D.AMBIENT + D.INTENSITY * (DC.FLOOR_Z - lamp[2]) / np.linalg.norm(l) ** 3        # n = (0, 0, -1): c = (z_floor - z_lamp) / |l|
        assert np.allclose(w["linear"][0, yi, xi].numpy(), alb * E, rtol=1e-6, atol=0), (yi, xi)
    bg = torch.tensor(op["background"], dtype=torch.float64)
    assert bool((w["linear"][~w["hit"]] == bg).all()) and not bool(w["hit"][0, 0, 0])
    # the lamp's size bounds the irradiance: a lamp 1 cm above the floor lights it as one 10 cm above would
    near = dict(op, light_cam=torch.tensor([[0.2, -0.1, DC.FLOOR_Z - 0.01]], dtype=torch.float64))
    peak = float(DC.reference(near, 1)["linear"].max())
    assert peak <= float(alb.max()) * (D.AMBIENT + D.INTENSITY / D.LIGHT_SIZE ** 2) * (1 + 1e-12)


def test_occluder_casts_the_lamp_projected_square():
    op, w = DC.operands("occluder"), DC.want("occluder")
    S, lamp = op["S"], np.asarray(DC.LAMP)
    cx, cy, z, half = DC.OCCLUDER
    reach = half * (DC.FLOOR_Z - lamp[2]) / (z - lamp[2])                    # the umbra's half side on the floor: 0.4
    assert abs(reach - 0.4) < 1e-12
    inside = outside = on_top = 0
    for yi in range(S):
        for xi in range(S):
            f = int(op["face_index"][0, yi, xi])
            if f < 0:
                continue
            if f >= 2:                                                       # the occluder itself faces the lamp: lit
                assert bool(w["visible"][0, yi, xi]); on_top += 1
                continue
            p = _sample_point(S, yi, xi, DC.FLOOR_Z)
            far = max(abs(p[0] - cx), abs(p[1] - cy))
            if far < reach - 1e-3:
                assert not bool(w["visible"][0, yi, xi]), (yi, xi); inside += 1
            elif far > reach + 1e-3:
                assert bool(w["visible"][0, yi, xi]), (yi, xi); outside += 1
    assert inside >= 10 and outside >= 300 and on_top >= 10
    lit = DC.want("floor")["linear"]
    dark = ~w["visible"][0] & (op["face_index"][0] < 2) & w["hit"][0]
    assert bool((w["linear"][0][dark] < lit[0][dark]).all())
    # a lamp behind the faces lights nothing: c = 0, the ambient term alone, and no ray is cast
    D = pkg("host.draw3d")
    b = DC.want("lamp_behind")
    lab = DC.operands("lamp_behind")["face_label"][0][DC.operands("lamp_behind")["face_index"][0].clamp(min=0).long()]
    assert bool(b["visible"].all()) and torch.allclose(b["linear"][b["hit"]], (D.albedo_table().double()[lab.long()] * D.AMBIENT)[b["hit"][0]], rtol=1e-12)


def _encode_numpy(linear, k):
    """the picture of ``linear`` [S, S, 3] written out sample by sample"""
    S = linear.shape[0]
    P = S // k
    out = np.zeros((P, P, 3), np.uint8)
    for Y in range(P):
        for X in range(P):
            acc = np.zeros(3, linear.dtype)
            for j in range(k):
                for i in range(k):
                    acc = acc + linear[Y * k + j, X * k + i]
            m = np.clip(acc / float(k * k), 0.0, 1.0)
            enc = np.where(m <= 0.0031308, 12.92 * m, 1.055 * np.maximum(m, 1e-30) ** (1.0 / 2.4) - 0.055)
            out[P - 1 - Y, X] = np.floor(enc * 255.0 + 0.5).astype(np.uint8)
    return out


@pytest.mark.parametrize("name", ["occluder", "chosen_by_hand", "five_views"])
def test_picture_is_the_encoded_box_filter_of_linear(name):
    D = pkg("host.draw3d")
    op, w = DC.operands(name), DC.want(name)
    for k in sorted(set(op["ks"]) | {1}):
        pic = D.encode_picture(w["linear"], k)
        assert pic.dtype == torch.uint8 and pic.shape == (w["linear"].shape[0], op["S"] // k, op["S"] // k, 3)
        for r in range(pic.shape[0]):
            assert np.array_equal(pic[r].numpy(), _encode_numpy(w["linear"][r].numpy(), k)), (k, r)
    assert torch.equal(w["picture"], D.encode_picture(w["linear"], op["ks"][0])) and int(w["picture"].max()) > int(w["picture"].min())
    # above 1 the mean is clamped: byte 255
    assert D.encode_picture(torch.full((1, 2, 2, 3), 7.0, dtype=torch.float64), 2).flatten().tolist() == [255] * 3


def test_without_shadows_every_sample_sees_the_lamp():
    for name in ("occluder", "five_views"):
        op, w = DC.operands(name), DC.want(name)
        off = DC.reference(op, op["ks"][0], shadows=False)
        dark = w["hit"] & ~w["visible"]
        assert bool(off["visible"].all()) and int(dark.sum()) > 0 and torch.equal(off["hit"], w["hit"])
        assert torch.equal(off["linear"][~dark], w["linear"][~dark]) and bool((off["linear"][dark].sum(-1) > w["linear"][dark].sum(-1)).all())


def test_fp32_restatement_stays_inside_the_figure_the_kernel_is_allowed_four_times_of():
    """Both precisions of ``draw3d_torch`` on the SAME operands - the float64 route's faces as the rasterizer saw them (float32) and its
    maps -, so that only the shading arithmetic differs (two rasterisations would disagree about the face of an edge sample)."""
    import test_draw3d_gpu as G
    worst = 0.0
    for name in DC.ROOMS:
        op, w = DC.operands(name), DC.want(name)
        got = DC.reference(op, op["ks"][0], dtype=torch.float32)
        err, unsafe, hits = DC.linear_error(got["linear"], w)
        flips = int(((got["visible"] != w["visible"]) & w["hit"] & ~w["unsafe"]).sum())
        dark = float((w["hit"] & ~w["visible"]).sum()) / max(hits, 1)
        print("%s: fp32 torch against fp64 on %d hit samples, largest |d| / max(1, |want|) = %.3e; unsafe %.4f %%, shadowed %.2f %%"
              % (name, hits, err, 100 * unsafe, 100 * dark))
        assert got["linear"].dtype == torch.float32 and flips == 0 and unsafe <= DC.UNSAFE_CAP, name
        worst = max(worst, err)
        if name == "every_face_culled":
            assert hits == 0 and op["status"].tolist() == [1]
        else:
            assert hits > 0
        if name == "five_views":
            assert 0.02 <= dark <= 0.98, "shadows are not exercised"
    print("largest: %.3e (FP32_TORCH_ERR %.3e)" % (worst, G.FP32_TORCH_ERR))
    assert worst <= G.FP32_TORCH_ERR <= 2.0 * worst


def test_hand_made_cases_meet_the_conditions_the_gpu_test_relies_on():
    for name in DC.HAND:
        op, w = DC.operands(name), DC.want(name)
        _, unsafe, hits = DC.linear_error(w["linear"], w)
        assert hits > 0 and unsafe <= DC.UNSAFE_CAP, name
        F = op["faces_xyz"].shape[1]
        if name.startswith("soup_"):
            assert F == int(name[5:]) and 0.1 < float((w["hit"] & ~w["visible"]).sum()) / hits < 0.9
    assert sorted(int(n[5:]) for n in DC.HAND if n.startswith("soup_")) == [200, DC.CHUNK - 1, DC.CHUNK, DC.CHUNK + 1, 600] and 600 > 2 * DC.CHUNK
    op, w = DC.operands("index_outside"), DC.want("index_outside")
    F = op["faces_xyz"].shape[1]
    assert {-1, F, F + 1000} <= set(op["face_index"].flatten().tolist())
    assert not bool(w["hit"][0, 3].any()) and not bool(w["hit"][0, op["S"] // 2, op["S"] // 2]) and bool((w["linear"][~w["hit"]] == 0).all())
    op, w = DC.operands("label_above_40"), DC.want("label_above_40")
    big = (op["face_label"][0][op["face_index"][0].clamp(min=0).long()] > 40) & w["hit"][0]
    assert int(big.sum()) > 20 and bool((w["linear"][0][big] == 0).all()) and bool((w["linear"][0][w["hit"][0] & ~big] > 0).any())
    op, w = DC.operands("chosen_by_hand"), DC.want("chosen_by_hand")
    assert op["chosen"].tolist() == [2, 1] and not torch.equal(w["linear"][0], w["linear"][1])
    assert torch.equal(w["linear"][0], DC.want("occluder")["linear"][0])


def _host_operands(R=1, V=2, F=4, S=8):
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return dict(faces_xyz=f32(R * V, F, 3, 3), face_index=torch.zeros(R * V, S, S, dtype=torch.int32), depth=f32(R * V, S, S),
                face_label=torch.zeros(R, F, dtype=torch.uint8), chosen=torch.zeros(R, dtype=torch.int64), K=f32(R * V, 3, 3), light_cam=f32(R, 3),
                albedo=f32(41, 3))


def test_argument_checks_refuse_before_any_launch():
    """every refusal returns before a launch: host tensors stand in for the device buffers, none is read"""
    D, L = pkg("host.draw3d"), pkg("_lib")
    assert len(L.SIGNATURES["sln_draw3d"][1]) == 5 and len(L.SIGNATURES["sln_draw3d_workspace_bytes"][1]) == 2
    lib = L.lib()
    assert lib.sln_draw3d_workspace_bytes(3, 100) == 3 * (100 * 64 + 32) and lib.sln_draw3d_workspace_bytes(2, 257) == 2 * (257 * 64 + 2 * 32) and lib.sln_draw3d_workspace_bytes(0, 5) < 0 and lib.sln_draw3d_workspace_bytes(1, 0) < 0
    assert lib.sln_draw3d_workspace_bytes(1, (1 << 24) + 1) < 0

    def refused(k=2, ws_offset=0, drop=None, **shape):
        op = _host_operands(**shape)
        S = op["face_index"].shape[1]
        ws = torch.zeros(16 * 64 + 4, dtype=torch.float32)
        ws = ws[(-(ws.data_ptr() // 4) % 4 + ws_offset):]                   # 16-byte aligned, then moved by ws_offset floats
        pic = torch.zeros(op["face_label"].shape[0], max(S // max(k, 1), 1), max(S // max(k, 1), 1), 3, dtype=torch.uint8)
        with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
            if drop is not None:
                d = L.SlnDraw3D()
                for key in ("faces_xyz", "face_index", "depth", "face_label", "chosen", "K", "light_cam", "albedo"):
                    setattr(d, key, None if key == drop else op[key].data_ptr())
                d.R, d.V, d.F, d.S, d.k, d.shadows = 1, 2, 4, S, k, 1
                L.check(lib.sln_draw3d(d, None if drop == "workspace" else L.ptr(ws), None if drop == "picture" else L.ptr(pic), None, None), "sln_draw3d")
            else:
                D.draw3d_launch(**dict(op, k=k, workspace=ws, picture=pic))

    for key in ("faces_xyz", "face_index", "depth", "face_label", "chosen", "K", "light_cam", "albedo", "picture", "workspace"):
        refused(drop=key)
    refused(k=3)                                  # S % k != 0
    refused(k=0)
    refused(k=17, S=34)                           # k > 16
    refused(ws_offset=1)                          # misaligned workspace
    refused(R=257, V=256, F=1, S=2, k=1)          # R * V > 65535
    with pytest.raises(L.SlnError, match="SLN_E_BADARG"):
        L.check(lib.sln_draw3d(None, None, None, None, None), "sln_draw3d")


def test_draw3d_has_no_cpu_fallback():
    D, L = pkg("host.draw3d"), pkg("_lib")
    with pytest.raises(L.SlnError, match="no CPU fallback.*draw3d_torch"):
        D.Draw3D(types.SimpleNamespace(device="cpu", size=64, views=5, batch=1))
