"""csrc/mesh_split.hip through host/mesh_prep.py against the rule's numpy restatement (``split_long_edges_np``) for EQUALITY - vertex
bits, faces, origins, passes - on every case of tests/mesh_split_cases.py, and ``MeshBank.from_arrays(max_edge=)`` through the scene
pass."""

import numpy as np
import pytest
import torch

import mesh_split_cases as MC
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = MC.cases()
NAMES = sorted(CASES)
_REF = {}


def ref(name):
    """the restatement's result, computed once per case and left unchanged"""
    if name not in _REF:
        _REF[name] = pkg("host.mesh_prep").split_long_edges_np(*CASES[name], MC.MAX_EDGE)
    return _REF[name]


def on_device(name):
    v, f = CASES[name]
    return torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()


def assert_equal(got, want, what):
    (v, f, info), (v1, f1, i1) = got, want
    assert v.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32 and info["origin"].dtype == torch.int32, what
    assert v.cpu().numpy().tobytes() == v1.tobytes(), what
    assert np.array_equal(f.cpu().numpy(), f1), what
    assert np.array_equal(info["origin"].cpu().numpy(), i1["origin"]), what
    assert info["passes"] == i1["passes"] and info["longest_in"] == i1["longest_in"], what


@pytest.mark.parametrize("name", NAMES)
def test_device_result_equals_the_restatement(name):
    MP = pkg("host.mesh_prep")
    got = MP.split_long_edges(*on_device(name), MC.MAX_EDGE)
    assert got[2]["status"] == 0
    assert_equal(got, ref(name), name)


@pytest.mark.parametrize("name", ["soup_257", "wall_slab"])
def test_a_second_call_gives_the_same_bytes_whatever_the_deterministic_switch_says(name):
    MP, L = pkg("host.mesh_prep"), pkg("_lib").lib()
    runs = []
    was = L.sln_get_deterministic()
    try:
        for on in (0, 1, 0):
            L.sln_set_deterministic(on)
            v, f, info = MP.split_long_edges(*on_device(name), MC.MAX_EDGE)
            runs.append((v.cpu().numpy().tobytes(), f.cpu().numpy().tobytes(), info["origin"].cpu().numpy().tobytes(), info["passes"]))
    finally:
        L.sln_set_deterministic(was)
    assert runs[0] == runs[1] == runs[2]


def test_a_face_outside_the_table_comes_through_unsplit_with_the_status_bit():
    MP = pkg("host.mesh_prep")
    v, f = CASES["soup_40_60"]
    bad = {7: (3, 40, 5), 20: (-1, 2, 3), 59: (1, 2, 2 ** 31 - 1)}
    g = f.copy()
    for k, tri in bad.items():
        g[k] = tri
    with pytest.raises(IndexError):
        MP.split_long_edges(torch.from_numpy(v).cuda(), torch.from_numpy(g).cuda(), MC.MAX_EDGE)
    vo, fo, info = MP.split_long_edges(torch.from_numpy(v).cuda(), torch.from_numpy(g).cuda(), MC.MAX_EDGE, validate=False)
    assert info["status"] == MP.STATUS_BAD_FACE
    fo, origin = fo.cpu().numpy(), info["origin"].cpu().numpy()
    for k, tri in bad.items():
        assert fo[origin == k].tolist() == [list(tri)]
    # one launch of the marking kernel on the same faces: mask 0, one child, no key, word 0 of the status
    L = pkg("_lib")
    dv, dg = torch.from_numpy(v).cuda(), torch.from_numpy(g).cuda()
    F = g.shape[0]
    mask, count, status = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (F, F, 4))
    status.zero_()
    keys = torch.full((F, 3), -7, dtype=torch.int64, device="cuda")
    assert L.lib().sln_mesh_split_mark(L.ptr(dv), v.shape[0], L.ptr(dg), F, MC.MAX_EDGE ** 2, L.ptr(mask), L.ptr(count), L.ptr(keys),
                                       L.ptr(status), L.current_stream_ptr()) == 0
    rows = list(bad)
    assert mask[rows].tolist() == [0, 0, 0] and count[rows].tolist() == [1, 1, 1] and bool((keys[rows] == -1).all())
    assert status.tolist() == [1, 0, 0, 0] and bool((count >= 1).all()) and bool((mask >= 0).all())
    # every other face: the restatement on the mesh without the three (they mark no edge, so the keys are the same)
    good = np.array([k for k in range(f.shape[0]) if k not in bad])
    v1, f1, i1 = MP.split_long_edges_np(v, f[good], MC.MAX_EDGE)
    rest = ~np.isin(origin, list(bad))
    assert vo.cpu().numpy().tobytes() == v1.tobytes()
    assert np.array_equal(fo[rest], f1) and np.array_equal(origin[rest], good[i1["origin"]]) and info["passes"] == i1["passes"]


def test_split_meshes_of_all_cases_at_once_equals_each_case_alone():
    MP = pkg("host.mesh_prep")
    got = MP.split_meshes([on_device(n) for n in NAMES], MC.MAX_EDGE)
    for name, g in zip(NAMES, got):
        assert g[2]["status"] == 0
        assert_equal(g, ref(name), name)


def test_badarg_refusals_launch_nothing():
    L = pkg("_lib")
    lib, P, st = L.lib(), L.ptr, L.current_stream_ptr
    v, f = on_device("cube_1")
    V, F = int(v.shape[0]), int(f.shape[0])
    SENT = 0x5A5A5A5A
    mask, count, status = (torch.full((n,), SENT, dtype=torch.int32, device="cuda") for n in (F, F, 4))
    keys = torch.full((F, 3), SENT, dtype=torch.int64, device="cuda")
    ok = [P(v), V, P(f), F, 0.36, P(mask), P(count), P(keys), P(status), st()]

    def mark(**kw):
        a = list(ok)
        for k, x in kw.items():
            a[int(k[1:])] = x
        return lib.sln_mesh_split_mark(*a)

    for at in (0, 2, 5, 6, 7, 8):
        assert mark(**{"a%d" % at: None}) == -1
    assert mark(a1=0) == -1 and mark(a3=0) == -1 and mark(a1=-3) == -1 and mark(a3=-1) == -1
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert mark(a4=thr) == -1
    assert mark(a1=2 ** 31 - 3 * F) == -1                       # V + 3 F = 2^31
    vn = torch.full((5, 3), 7.0, device="cuda")
    uk = torch.tensor([1, (1 << 32) | 2], dtype=torch.int64, device="cuda")
    assert lib.sln_mesh_split_midpoints(None, V, P(uk), 2, P(vn), P(status), st()) == -1
    assert lib.sln_mesh_split_midpoints(P(v), V, P(uk), 0, P(vn), P(status), st()) == -1
    assert lib.sln_mesh_split_midpoints(P(v), 0, P(uk), 2, P(vn), P(status), st()) == -1
    fo, oo = torch.full((4 * F, 3), SENT, dtype=torch.int32, device="cuda"), torch.full((4 * F,), SENT, dtype=torch.int32, device="cuda")
    off = torch.arange(F, dtype=torch.int64, device="cuda")
    mid = torch.full((F, 3), -1, dtype=torch.int32, device="cuda")
    zero = torch.zeros(F, dtype=torch.int32, device="cuda")
    emit = [P(v), V, 0, P(f), P(zero), P(zero), P(off), P(mid), F, F, P(fo), P(oo), P(status), st()]
    for at, x in ((0, None), (3, None), (6, None), (10, None), (1, 0), (2, -1), (8, 0), (9, F - 1), (9, 4 * F + 1)):
        a = list(emit); a[at] = x
        assert lib.sln_mesh_split_emit(*a) == -1
    torch.cuda.synchronize()
    for t in (mask, count, status, keys, fo, oo):
        assert bool((t == SENT).all())
    assert bool((vn == 7.0).all())


def test_a_quad_shell_room_gets_its_ceiling_through_the_scene_pass_once_split():
    """tests/test_mesh_split_host.py states the camera-depth argument: both triangles of a one-quad ceiling have a corner behind the
    camera and collapse; split to 0.6 the far part of the ceiling is drawn."""
    R = pkg("host.refine"); DR = pkg("host.diff_render")
    names, boxes, angles, meshes = MC.quad_room_inputs()
    boxes, angles = torch.from_numpy(boxes).cuda(), torch.from_numpy(angles).cuda()
    plane = 1 + DR.nyu_class.index("ceiling")
    pixels = {}
    for max_edge in (None, 0.6):
        bank = R.MeshBank.from_arrays(meshes, "cuda", shell=MC.quad_room(), max_edge=max_edge)
        scene = R.RefineScene(names, bank, boxes[-1].clone(), image_size=96)
        with torch.no_grad():
            target = scene.render(boxes, angles)[0]
        pixels[max_edge] = int((target[0, plane] > 0.5).sum())
        if max_edge is None:
            continue
        assert bank.models["bed"]["f"].shape[0] > 12 and bank.models["bed"]["f"].is_cuda
        b = (boxes + 0.02).detach().requires_grad_(True)
        a = (angles + 0.7).detach().requires_grad_(True)
        sizes = scene.render(boxes, angles)[2].detach()
        img, size_loss, _ = scene.render(b, a, sizes)
        loss, _, _ = R.refinement_loss(img, target, R.target_labels(target), size_loss)
        loss.backward()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(b.grad).all()) and bool(torch.isfinite(a.grad).all())
        assert float(b.grad[:-1].abs().max()) > 0
    assert pixels[None] == 0 and pixels[0.6] > 0
