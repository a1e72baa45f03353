"""The edge splitter's rule in numpy (host/mesh_prep.py::split_long_edges_np: the CPU route, and what tests/test_mesh_split_gpu.py holds
the kernels to): properties any correct splitter has, the figures of DESIGN §4's table, the error paths, and what
``MeshBank.from_arrays(max_edge=)`` does with it.  No GPU."""
import math

import numpy as np
import pytest
import torch

import mesh_split_cases as MC
from conftest import pkg

CASES = MC.cases()
NAMES = sorted(CASES)
_RESULTS = {}


def split(name):
    """one run per case, shared and left unchanged"""
    if name not in _RESULTS:
        v, f = CASES[name]
        _RESULTS[name] = pkg("host.mesh_prep").split_long_edges_np(v, f, MC.MAX_EDGE)
    return _RESULTS[name]


def edge_sq(v, f):
    p = v.astype(np.float64)[f.astype(np.int64)]                # [F, 3, 3]
    d = p - p[:, [1, 2, 0]]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def cross2(v, f):
    """twice the area vector of every face, float64 - exact on the cases' coordinates"""
    p = v.astype(np.float64)[f.astype(np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def issue_bound(longest, max_edge):
    return max(0, int(math.ceil(math.log(longest / max_edge) / math.log(2.0 / math.sqrt(3.0)))))


@pytest.mark.parametrize("name", NAMES)
def test_no_output_edge_is_longer_than_max_edge_and_passes_stay_within_the_bound(name):
    v, f = CASES[name]
    vo, fo, info = split(name)
    assert vo.dtype == np.float32 and fo.dtype == np.int32 and info["origin"].shape == (fo.shape[0],)
    assert fo.min() >= 0 and fo.max() < vo.shape[0]
    assert edge_sq(vo, fo).max() <= MC.MAX_EDGE * MC.MAX_EDGE
    assert info["longest_in"] == math.sqrt(edge_sq(v, f).max())
    assert info["passes"] <= issue_bound(info["longest_in"], MC.MAX_EDGE)
    assert np.array_equal(vo[:v.shape[0]], v)                                          # old vertices keep their indices
    assert np.all(np.diff(info["origin"]) >= 0) and set(info["origin"].tolist()) == set(range(f.shape[0]))   # input face order


@pytest.mark.parametrize("name", sorted(MC.CUBOIDS))
def test_cuboids_match_the_prototype_table_and_stay_closed_with_exact_area(name):
    _, passes, faces, verts = MC.CUBOIDS[name]
    v, f = CASES[name]
    vo, fo, info = split(name)
    assert (info["passes"], fo.shape[0], vo.shape[0]) == (passes, faces, verts)
    # every undirected edge of the closed surface is used by exactly two faces
    e = np.sort(np.concatenate([fo[:, [0, 1]], fo[:, [1, 2]], fo[:, [2, 0]]]), 1)
    _, n = np.unique(e, axis=0, return_counts=True)
    assert (n == 2).all()
    # twice the area per origin, exactly: axis-aligned faces have one non-zero cross component, and dyadic sums are exact
    c = cross2(vo, fo)
    assert ((c != 0).sum(1) == 1).all()
    got = np.zeros(f.shape[0])
    np.add.at(got, info["origin"], np.abs(c).sum(1))
    assert np.array_equal(got, np.abs(cross2(v, f)).sum(1))


@pytest.mark.parametrize("name", NAMES)
def test_winding_is_kept(name):
    v, f = CASES[name]
    vo, fo, info = split(name)
    parent, child = cross2(v, f)[info["origin"]], cross2(vo, fo)
    flat = ~parent.any(1)
    assert not child[flat].any()                                                       # a face without area has no child with one
    assert ((parent[~flat] * child[~flat]).sum(1) > 0).all()


def test_unwelded_coincident_triangles_get_bit_identical_midpoints():
    vo, fo, info = split("unwelded_pair")
    sides = [set(map(bytes, vo[np.unique(fo[info["origin"] == k])])) for k in (0, 1)]
    assert len(sides[0]) > 3 and sides[0] == sides[1]
    assert not set(np.unique(fo[info["origin"] == 0])) & set(np.unique(fo[info["origin"] == 1]))          # and stay unwelded


@pytest.mark.parametrize("rot", range(3))
@pytest.mark.parametrize("which, rest", [("a", [(0, 1, 4), (0, 4, 3)]), ("b", [(0, 1, 3), (1, 4, 3)]), ("tie", [(0, 1, 4), (0, 4, 3)])])
def test_two_marked_edges_cut_the_quad_by_the_shorter_diagonal_and_a_tie_goes_to_a_m1(which, rest, rot):
    """max_edge = 0.75 ends these after one pass.  A, B, C are vertices 0, 1, 2 wherever the face starts; the keys (0,2) < (1,2) make
    M2 = mid(C, A) vertex 3 and M1 = mid(B, C) vertex 4.  (M2, M1, C) comes first, then the quad: `a` has |A M1| shorter, `b` |B M2|,
    `tie` both equal."""
    v, f = CASES["tri_2_marked_%s_k%d" % (which, rot)]
    vo, fo, info = pkg("host.mesh_prep").split_long_edges_np(v, f, 0.75)
    assert info["passes"] == 1
    assert np.array_equal(vo[3:], np.stack([(v[2] + v[0]) / 2, (v[1] + v[2]) / 2]))
    assert fo.tolist() == [[3, 4, 2]] + [list(t) for t in rest]
    dA, dB = ((vo[0].astype(np.float64) - vo[4]) ** 2).sum(), ((vo[1].astype(np.float64) - vo[3]) ** 2).sum()
    assert {"a": dA < dB, "b": dA > dB, "tie": dA == dB}[which]


@pytest.mark.parametrize("rot", range(3))
def test_one_and_three_marked_edges_emit_the_stated_children(rot):
    MP = pkg("host.mesh_prep")
    v, f = CASES["tri_1_marked_k%d" % rot]
    vo, fo, info = MP.split_long_edges_np(v, f, MC.MAX_EDGE)
    assert info["passes"] == 1 and fo.tolist() == [[0, 3, 2], [3, 1, 2]] and np.array_equal(vo[3], (v[0] + v[1]) / 2)
    v, f = CASES["tri_3_marked"]
    vo, fo, info = MP.split_long_edges_np(v, f, 0.75)                                  # keys (0,1) < (0,2) < (1,2): m0 = 3, m2 = 4, m1 = 5
    assert info["passes"] == 1 and fo.tolist() == [[0, 3, 4], [3, 1, 5], [4, 5, 2], [3, 5, 4]]


def test_a_mesh_that_needs_no_split_comes_back_unchanged():
    for name in ("no_split", "tri_0_marked"):
        v, f = CASES[name]
        vo, fo, info = split(name)
        assert info["passes"] == 0 and info["status"] == 0
        assert np.array_equal(vo, v) and np.array_equal(fo, f) and np.array_equal(info["origin"], np.arange(f.shape[0]))


def test_split_meshes_equals_the_per_mesh_results():
    MP = pkg("host.mesh_prep")
    empty = (np.zeros((3, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32))
    got = MP.split_meshes([CASES[n] for n in NAMES[:5]] + [empty] + [CASES[n] for n in NAMES[5:]], MC.MAX_EDGE)
    assert got[5][1].shape == (0, 3) and got[5][2]["passes"] == 0
    del got[5]
    for name, (vo, fo, info) in zip(NAMES, got):
        v1, f1, i1 = split(name)
        assert vo.tobytes() == v1.tobytes() and np.array_equal(fo, f1) and fo.dtype == np.int32, name
        assert np.array_equal(info["origin"], i1["origin"]) and info["passes"] == i1["passes"], name
        assert info["longest_in"] == i1["longest_in"]


def test_host_tensors_take_the_numpy_route_and_come_back_as_tensors():
    MP = pkg("host.mesh_prep")
    v, f = CASES["cube_1"]
    vo, fo, info = MP.split_long_edges(torch.from_numpy(v), torch.from_numpy(f), MC.MAX_EDGE)
    v1, f1, i1 = split("cube_1")
    assert isinstance(vo, torch.Tensor) and torch.equal(vo, torch.from_numpy(v1)) and torch.equal(fo, torch.from_numpy(f1))
    assert torch.equal(info["origin"], torch.from_numpy(i1["origin"])) and info["passes"] == 2
    va, fa, _ = MP.split_long_edges(v, f)                                              # arrays in, arrays out; 0.6 is the default
    assert isinstance(va, np.ndarray) and np.array_equal(va, v1) and np.array_equal(fa, f1)


def test_error_paths():
    MP = pkg("host.mesh_prep")
    v, f = CASES["cube_1"]
    bad = v.copy(); bad[3, 1] = np.nan
    for fn in (MP.split_long_edges, MP.split_long_edges_np):
        with pytest.raises(ValueError):
            fn(bad, f, 0.6)
        for me in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn(v, f, me)
        for wrong in (8, -1):
            g = f.copy(); g[5, 2] = wrong
            with pytest.raises(IndexError):
                fn(v, g, 0.6)
        with pytest.raises(ValueError, match="max_faces"):
            fn(*CASES["room_box"], 0.6, max_faces=1000)
    with pytest.raises(IndexError):
        MP.split_meshes([CASES["cube_1"], (v, f + 1)], 0.6)
    # a max_edge below the float32 spacing of the coordinates: the midpoint of two neighbouring floats is one of them, so an edge
    # never gets shorter - the pass bound ends it
    u = 2.0 ** -19                                                                     # the spacing at 16
    with pytest.raises(RuntimeError, match="passes"):
        MP.split_long_edges_np(np.array([(16, 0, 0), (16 + u, 0, 0)], dtype=np.float32), np.array([(0, 1, 1)]), u / 4)


def _bank(max_edge, shell=True, device="cpu"):
    R = pkg("host.refine")
    names, boxes, angles, meshes = MC.quad_room_inputs()
    meshes = dict(meshes, bed=[meshes["bed"] + (None, None, "bed_long"), MC.cuboid(1.0, 1.0, 1.0) + ((0, 0, 0), (1, 1.5, 1), "bed_cube")])
    kw = {} if max_edge == "absent" else dict(max_edge=max_edge)
    return R.MeshBank.from_arrays(meshes, device, shell=MC.quad_room() if shell else None, **kw), meshes


def test_from_arrays_without_max_edge_holds_the_arrays_of_today_and_with_it_keeps_boxes_ids_and_table():
    plain, meshes = _bank("absent")
    none, _ = _bank(None)
    fine, _ = _bank(0.6)
    room = MC.quad_room()
    for bank in (plain, none):
        for k, e in enumerate(bank.model_list("bed")):
            assert np.array_equal(e["v"].numpy(), meshes["bed"][k][0]) and np.array_equal(e["f"].numpy(), meshes["bed"][k][1])
        assert np.array_equal(bank.models["table"]["f"].numpy(), meshes["table"][1])
        for key in ("wall_v", "floor_v", "ceil_v", "floor_f", "ceil_f"):
            assert np.array_equal(bank.shell[key], room[key]), key
        assert all(np.array_equal(a, b) for a, b in zip(bank.shell["wall_f"], room["wall_f"]))
    MP = pkg("host.mesh_prep")
    for name in ("bed", "table"):
        for a, b in zip(plain.model_list(name), fine.model_list(name)):
            assert torch.equal(a["bbox_min"], b["bbox_min"]) and torch.equal(a["bbox_max"], b["bbox_max"]) and a["id"] == b["id"]
            assert np.array_equal(a["lo64"], b["lo64"]) and np.array_equal(a["hi64"], b["hi64"])
            v1, f1, _ = MP.split_long_edges_np(a["v"].numpy(), a["f"].numpy(), 0.6)
            assert np.array_equal(b["v"].numpy(), v1) and np.array_equal(b["f"].numpy(), f1) and b["f"].dtype == torch.int32
            assert f1.shape[0] > a["f"].shape[0]
    assert plain.table.ids == fine.table.ids and np.array_equal(plain.table.ratio_host, fine.table.ratio_host)
    assert all(torch.equal(a, b) for a, b in zip(plain.shell_ratios, fine.shell_ratios))
    # the wall is one mesh over wall_v; every sub-mesh keeps its own faces' children
    sh = fine.shell
    v1, f1, i1 = MP.split_long_edges_np(room["wall_v"], np.concatenate(room["wall_f"]), 0.6)
    assert np.array_equal(sh["wall_v"], v1) and len(sh["wall_f"]) == 3
    for k, sub in enumerate(sh["wall_f"]):
        assert np.array_equal(sub, f1[(i1["origin"] >= 2 * k) & (i1["origin"] < 2 * k + 2)]) and sub.shape[0] > 2
    for part in ("floor", "ceil"):
        v1, f1, _ = MP.split_long_edges_np(room[part + "_v"], room[part + "_f"], 0.6)
        assert np.array_equal(sh[part + "_v"], v1) and np.array_equal(sh[part + "_f"], f1)
        assert np.array_equal(v1.min(0), room[part + "_v"].min(0)) and np.array_equal(v1.max(0), room[part + "_v"].max(0))


def test_a_quad_ceiling_is_culled_whole_and_survives_once_split():
    """The refinement camera stands at (X/2, Y/2 + 0.1, Z), looks along -z and down by 0.4 rad (``get_cam_mat``), so the camera depth of
    a point is  -sin(0.4) (y - Y/2 - 0.1) - cos(0.4) (z - Z).  A ceiling corner at z = Z has depth -sin(0.4) (Y/2 - 0.1) < 0, and
    both triangles of a one-quad ceiling have such a corner: ``cull_and_classify`` drops a face when ANY corner is nearer than
    CULL_EPS = 0.06, so no ceiling face survives.  Split to 0.6, the faces with every corner at
    z <= Z - (0.06 + sin(0.4) (Y/2 - 0.1)) / cos(0.4)  (4.39 of 5 here) survive."""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    names, boxes, angles, _ = MC.quad_room_inputs()
    boxes, angles = torch.from_numpy(boxes), torch.from_numpy(angles)
    X, Y, Z = boxes[-1, 3:].tolist()
    K, Rm, t = DR.get_cam_mat(boxes[-1], "cpu")
    # the geometry first: the depth of the ceiling's corners as the camera matrices give it, against the formula above
    corners = torch.tensor([[0, Y, Z], [X, Y, Z], [0, Y, 0], [X, Y, 0]])
    depth = (torch.matmul(corners[None], Rm.transpose(1, 2)) + t)[0, :, 2]
    want = -math.sin(0.4) * (Y / 2 - 0.1) - math.cos(0.4) * (corners[:, 2] - Z)
    assert torch.allclose(depth, want.float(), atol=1e-5)
    assert depth[0] < 0 and depth[1] < 0 and depth[2] > DR.CULL_EPS and depth[3] > DR.CULL_EPS
    z_ok = Z - (DR.CULL_EPS + math.sin(0.4) * (Y / 2 - 0.1)) / math.cos(0.4)
    assert 0.6 < z_ok < Z - 0.6                                                         # room for whole faces on either side
    kept = {}
    for max_edge in (None, 0.6):
        bank, _ = _bank(max_edge)
        v, f, ranges, _, _ = R.assemble_scene(boxes, angles, names, bank, boxes[-1])
        (a, b), = ranges["ceiling"]
        assert b - a == (2 if max_edge is None else bank.shell["ceil_f"].shape[0])
        cv = v[0][f[0, a:b].long().reshape(-1)]
        assert bool((cv[:, 1] == Y).all()) and float(cv[:, 2].max()) == Z and float(cv[:, 2].min()) == 0.0      # the ceiling is where we think
        _, cls, classes, _, _ = DR.cull_and_classify(v, f, ranges, Rm, t)
        kept[max_edge] = int((cls == classes.index("ceiling")).sum())
        if max_edge is not None:
            far = (cv[:, 2].reshape(-1, 3) <= z_ok - 1e-4).all(1)
            assert kept[max_edge] >= int(far.sum()) > 0
    assert kept[None] == 0 and kept[0.6] > 0
