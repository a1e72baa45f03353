"""Mesh retrieval, host side (host/retrieve.py; CPU-only): the torch restatement against the choices the reference's own
``suncg_retrieve`` / ``wall_retrieve`` / ``floor_retrieve`` made (tests/golden/mesh_retrieve.npz, tools/gen_golden_mesh_retrieve.py), the
reference-shaped wrappers, the table's CSR, and the bank / scene assembly that take the choice."""
import numpy as np
import pytest
import torch

from conftest import load_golden, pkg


def golden_tables():
    """-> (npz, vocab, suncg_data-shaped dict, wall_data-shaped list) of the fixture"""
    g = load_golden("mesh_retrieve")
    vocab = bytes(g["vocab"]).decode().split("\n")
    ids = bytes(g["model_ids"]).decode().split("\n")
    data = {name: [] for name in vocab[1:]}
    for c, mid, bb in zip(g["model_class"], ids, g["model_bbox"]):
        data[vocab[int(c)]].append({"id": mid, "bbox_min": bb[0].tolist(), "bbox_max": bb[1].tolist()})
    wall = [{"wall_bbox_min": w[0].tolist(), "wall_bbox_max": w[1].tolist(), "floor_bbox_min": f[0].tolist(), "floor_bbox_max": f[1].tolist(), "index": j}
            for j, (w, f) in enumerate(zip(g["wall_bbox"], g["floor_bbox"]))]
    return g, vocab, data, wall


def test_restatement_equals_the_reference_choice_on_every_row():
    RT = pkg("host.retrieve")
    g, vocab, data, wall = golden_tables()
    table = RT.ModelTable(data, vocab)
    boxes, objs, room_row = torch.from_numpy(g["boxes"]), torch.from_numpy(g["objs"]), torch.from_numpy(g["room_row"])
    keep = boxes.clone()
    got, dist = RT.retrieve_models_torch(boxes, objs, room_row, table, dist=True)
    assert torch.equal(boxes, keep), "the caller's boxes were scaled in place"
    assert got.dtype == torch.int32 and int((got.numpy() != g["choice"]).sum()) == 0
    assert torch.equal(torch.isnan(dist), torch.from_numpy((g["choice"] < 0) | _nan_rows(g))), "dist is NaN exactly where nothing is chosen or every distance is"
    # S layouts of the same rows: every layout on its own
    alt = boxes.clone()
    obj_rows = room_row != torch.arange(len(room_row))
    alt[obj_rows, 4] = alt[obj_rows, 1] + 2.5 * (alt[obj_rows, 4] - alt[obj_rows, 1])
    layouts = RT.retrieve_models_torch(torch.stack([boxes, alt, boxes]), objs, room_row, table)
    assert torch.equal(layouts[0], got) and torch.equal(layouts[2], got) and torch.equal(layouts[1], RT.retrieve_models_torch(alt, objs, room_row, table))
    assert not torch.equal(layouts[1], got)
    wr, fr = (torch.from_numpy(x) for x in RT.shell_ratios(wall))
    sh = RT.retrieve_shell_torch(boxes, torch.from_numpy(g["last_row"]), wr, fr).numpy()
    assert int((sh[:, 0] != g["wall_choice"]).sum()) == 0 and int((sh[:, 1] != g["floor_choice"]).sum()) == 0
    # the fixture holds what it is there for (see the generator): first-of-duplicates, NaN rows, empty classes, both table forms of -1
    ch, ob = g["choice"], g["objs"]
    assert ((ob == vocab.index("lamp")) & (ch == -1)).sum() == 2 and (ch[ob == 0] == -1).all() and (ch[ob != 0][ob[ob != 0] != vocab.index("lamp")] >= 0).all()
    assert ((ob == vocab.index("slab")) & (ch == 2)).sum() >= 2
    assert 17 not in g["wall_choice"] and 21 not in g["wall_choice"]


def _nan_rows(g):
    """rows whose winning distance is a NaN: a zero-width box against a zero-width model (inf - inf), or a 0 / 0 box"""
    b, rr = g["boxes"], g["room_row"]
    with np.errstate(all="ignore"):
        ext = b[rr][:, 3:]
        d = b[:, 3:] * ext - b[:, :3] * ext
        zero_w = d[:, 0] == 0
    slab = g["objs"] == 6
    return (zero_w & slab) | (zero_w & (d[:, 1] == 0))


def test_reference_shaped_wrappers_return_the_golden_ids_and_dicts():
    RT = pkg("host.retrieve")
    g, vocab, data, wall = golden_tables()
    RT.configure(data, vocab, wall_data=wall)
    ids_of = {name: [e["id"] for e in v] for name, v in data.items()}
    row0 = 0
    for r, last in enumerate(g["last_row"].tolist()):
        n = last + 1 - row0
        objs = g["objs"][row0:last + 1].tolist()
        boxes = [torch.from_numpy(g["boxes"][i].copy()) for i in range(row0, last + 1)]
        want = g["choice"][row0:last + 1]
        if (want[:-1] < 0).any():
            with pytest.raises(ValueError):                     # the reference's np.argmin raises on a class without models
                RT.suncg_retrieve(objs, boxes)
        else:
            assert RT.suncg_retrieve(objs, boxes) == [ids_of[vocab[objs[i]]][want[i]] for i in range(n - 1)]
        assert all(torch.equal(b, torch.from_numpy(g["boxes"][row0 + i])) for i, b in enumerate(boxes))
        assert RT.wall_retrieve(boxes) is wall[g["wall_choice"][r]] and RT.floor_retrieve(boxes, wall) is wall[g["floor_choice"][r]]
        row0 = last + 1


def test_model_table_csr_with_empty_classes():
    RT = pkg("host.retrieve")
    data = {"b": [{"id": "b0", "bbox_min": [0, 0, 0], "bbox_max": [2, 1, 4]}, {"id": "b1", "bbox_min": [1, 1, 1], "bbox_max": [2, 4, 1.5]}],
            "d": [{"id": "d0", "bbox_min": [0.0, 0.0, 0.0], "bbox_max": [0.0, 1.0, 2.0]}], "c": []}
    t = RT.ModelTable(data, ["__room__", "a", "b", "c", "d", "e"])
    assert t.class_ptr.tolist() == [0, 0, 0, 2, 2, 3, 3] and t.n_classes == 6 and t.n_models == 3
    assert t.ids == [[], [], ["b0", "b1"], [], ["d0"], []] and [t.count(c) for c in range(6)] == [0, 0, 2, 0, 1, 0]
    assert t.ratio.dtype == torch.float64 and t.ratio[:2].tolist() == [[0.5, 2.0], [3.0, 0.5]] and torch.isinf(t.ratio[2]).all()
    assert t.id_of(2, 1) == "b1"
    empty = RT.ModelTable({}, ["__room__", "a"])
    assert empty.n_models == 0 and empty.ratio.shape == (0, 2)
    got = RT.retrieve_models_torch(torch.rand(3, 6), torch.tensor([1, 1, 0]), torch.tensor([2, 2, 2]), empty)
    assert got.tolist() == [-1, -1, -1]
    # a class outside the table, a room row, a class without models
    boxes = torch.tensor([[0, 0, 0, 1, 3, 0.5], [0, 0, 0, 1, 0.5, 2], [0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1], [0, 0, 0, 2, 2, 2]], dtype=torch.float32)
    got = RT.retrieve_models_torch(boxes, torch.tensor([2, 2, 9, 3, 0]), torch.full((5,), 4), t)
    assert got.tolist() == [1, 0, -1, -1, -1]


def _cuboid(lo, hi, subdiv):
    syn = pkg("host.synthetic")
    v, f = syn._grid_cuboid(np.asarray(lo, np.float64), np.asarray(hi, np.float64), subdiv)
    return v.astype(np.float32), f.astype(np.int32)


def many_model_bank(R, names, device):
    """three models per class: ratios (y/x, z/x) of (0.2, 1), (0.8, 1.25), (3, 1), with 1, 2 and 3 subdivisions (different vertex and
    face counts), every model's table box as large again as its vertices' (the scale is the table's)"""
    meshes = {}
    for c, name in enumerate(names):
        models = []
        for k, (size, sub) in enumerate(((np.array([1.0, 0.2, 1.0]), 1), (np.array([1.0, 0.8, 1.25]), 2), (np.array([0.5, 1.5, 0.5]), 3))):
            size = size * (1.0 + 0.1 * c)
            v, f = _cuboid(-size / 2, size / 2, sub)
            models.append((v, f, (-size).tolist(), size.tolist(), "%s_%d" % (name, k)))
        meshes[name] = models
    return R.MeshBank.from_arrays(meshes, device)


def test_bank_takes_one_model_or_a_list_per_class():
    R = pkg("host.refine")
    v, f = _cuboid([0, 0, 0], [1, 2, 3], 1)
    one = R.MeshBank.from_arrays({"bed": (v, f), "chair": (v, f, [0, 0, 0], [2, 2, 2]), "desk": {"v": v, "f": f}}, "cpu")
    assert not one.has_choice() and one.table.n_models == 3 and one.table.ids[one.table.vocab.index("bed")] == ["bed#0"]
    assert one.models["chair"]["bbox_max"].tolist() == [2.0, 2.0, 2.0] and len(one.model_list("bed")) == 1
    many = many_model_bank(R, ["bed", "chair"], "cpu")
    assert many.has_choice() and many.models["bed"] is many.model_list("bed")[0] and len(many.model_list("chair")) == 3
    t = many.table
    c = t.vocab.index("chair")
    assert t.count(c) == 3 and t.ids[c] == ["chair_0", "chair_1", "chair_2"] and t.vocab[0] == "__room__"
    np.testing.assert_array_equal(t.ratio_host[t.class_ptr_host[c]:t.class_ptr_host[c + 1]], [[0.2, 1.0], [0.8, 1.25], [3.0, 1.0]])
    assert [m["v"].shape[0] for m in many.model_list("bed")] == sorted(set(m["v"].shape[0] for m in many.model_list("bed")))
    with pytest.raises(ValueError, match="twice"):
        R.MeshBank.from_arrays({"bed": [(v, f, [0, 0, 0], [1, 2, 3], "x"), (v, f, [0, 0, 0], [1, 1, 1], "x")]}, "cpu")
    shell = dict(wall_v=v, wall_f=[f], wall_bbox=[[0, 0, 0], [1, 2, 3]], floor_v=v, floor_f=f, floor_bbox=[[0, 0, 0], [1, 2, 3]], ceil_v=v, ceil_f=f)
    shell2 = dict(shell, wall_bbox=[[0, 0, 0], [1, 1, 1]], floor_bbox=[[0, 0, 0], [1, 1, 2]])
    b1, b2 = R.MeshBank.from_arrays({"bed": (v, f)}, "cpu", shell=shell), R.MeshBank.from_arrays({"bed": (v, f)}, "cpu", shell=[shell, shell2])
    assert len(b1.shells) == 1 and b1.shell is b1.shells[0] and not b1.has_choice() and b2.has_choice() and b2.shell is b2.shells[0]
    assert b2.shell_ratios[0].tolist() == [[2.0, 3.0], [1.0, 1.0]] and b2.shell_ratios[1].tolist() == [3.0, 2.0]
    assert R.MeshBank.from_arrays({"bed": (v, f)}, "cpu").shell_ratios is None


def test_assemble_scene_places_the_chosen_model():
    R = pkg("host.refine")
    names = ["bed", "chair", "bed", "__room__"]
    bank = many_model_bank(R, ["bed", "chair"], "cpu")
    boxes = torch.tensor([[0.1, 0.0, 0.1, 0.2, 0.5, 0.18], [0.5, 0.0, 0.2, 0.8, 0.1, 0.5], [0.2, 0.0, 0.6, 0.5, 0.2, 0.9], [0, 0, 0, 4.0, 2.7, 5.0]])
    angles = torch.zeros(4)
    models, _ = R.retrieve_choice(bank, boxes, names)
    assert models.tolist() == [2, 0, 1, -1]                    # tall, flat, in between; the room row retrieves nothing
    v0, f0, ranges0, _, _ = R.assemble_scene(boxes, angles, names, bank, boxes[-1])
    v, f, ranges, sizes, _ = R.assemble_scene(boxes, angles, names, bank, boxes[-1], models=models.tolist())
    lists = [bank.model_list(n)[max(k, 0)] for n, k in zip(names[:-1], models.tolist())]
    n_shell = v0.shape[1] - 3 * 0 - sum(bank.models[n]["v"].shape[0] for n in names[:-1])
    assert v.shape[1] == sum(m["v"].shape[0] for m in lists) + n_shell and v.shape[1] != v0.shape[1]
    assert ranges["bed"] == [[0, lists[0]["f"].shape[0]], [lists[0]["f"].shape[0] + lists[1]["f"].shape[0], sum(m["f"].shape[0] for m in lists)]]
    at = 0
    for m, size in zip(lists, sizes):
        # scale = min(size / msize) of the CHOSEN entry's table box: the placed vertices span scale * (the mesh's own extent)
        scale = float((size / (m["bbox_max"] - m["bbox_min"])).min())
        span = v[0, at:at + m["v"].shape[0]].max(0).values - v[0, at:at + m["v"].shape[0]].min(0).values
        own = m["v"].max(0).values - m["v"].min(0).values
        np.testing.assert_allclose(span.numpy(), scale * own.numpy(), rtol=1e-5)
        at += m["v"].shape[0]
    # None and all-zero choices are today's scene
    vz, fz, _, _, _ = R.assemble_scene(boxes, angles, names, bank, boxes[-1], models=[0, 0, 0, -1])
    assert torch.equal(vz, v0) and torch.equal(fz, f0)
