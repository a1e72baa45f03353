"""Golden fixture for the mesh retrieval (host/retrieve.py, csrc/mesh_retrieve.hip), produced by EXECUTING THE REFERENCE'S OWN SOURCE TEXT
(needs the reference tree; build container only).

``suncg_retrieve`` (models/misc.py:34-64), ``wall_retrieve`` (:123-137) and ``floor_retrieve`` (:139-152) are taken out of the source text
with ``ast`` and ``exec``ed unmodified - the module itself cannot be imported (it parses options and pulls in pywavefront and pymesh).

What is injected (and therefore NOT pinned by this fixture): the module globals the three functions read - ``suncg_data``,
``object_idx_to_name`` and ``wall_data_json`` are the synthetic tables below (the licensed SUNCG tables are not here), and ``np`` is a
namespace that forwards to numpy and defines ``float`` as the builtin where this numpy no longer has the alias.  The functions get COPIES
of the boxes: ``suncg_retrieve`` scales the numpy view of ``box.cpu()`` in place, which for a host tensor is the caller's tensor.

The tables are built to hit what an argmin can get wrong: classes with 0, 1, 2 and 300 models; exact duplicates (the first one wins);
pairs whose ratios - hence distances - differ in the last float64 bits, in either table order; one model of zero width together with
zero-width boxes (a NaN distance wins; all-infinite and all-NaN rows keep index 0).  A class without models makes the reference raise
(np.argmin of an empty list, :62): the tool asserts that, runs the room without those rows and records -1 for them.

Before writing, the tool asserts that ``retrieve_models_torch`` / ``retrieve_shell_torch`` reproduce every recorded choice.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mesh_retrieve.py

Writes tests/golden/mesh_retrieve.npz (numeric arrays only; member times are fixed, so the file regenerates bit for bit).
"""
import importlib
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from oracle.gen_golden_refine import GOLD, REF, _run, _top_level      # noqa: E402

SRC = os.path.join(REF, "models/misc.py")
VOCAB = ["__room__", "bed", "chair", "desk", "lamp", "sofa", "slab", "shelf"]      # lamp: listed with no models; shelf: the last-bit pairs


def _numpy_namespace():
    ns = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    if not hasattr(ns, "float"):
        ns.float = float
    return ns


def _entry(name, k, size, lo=(0.0, 0.0, 0.0)):
    lo = np.asarray(lo, dtype=np.float64)
    return {"id": "%s_%03d" % (name, k), "bbox_min": [float(x) for x in lo], "bbox_max": [float(x) for x in lo + np.asarray(size, dtype=np.float64)]}


def tables(rng):
    data = {}
    data["bed"] = [_entry("bed", 0, (2.0, 0.6, 1.5)), _entry("bed", 1, (1.0, 0.5, 2.0), lo=(-0.5, 0.0, -1.0))]
    sizes = rng.uniform(0.3, 2.0, size=(300, 3))
    sizes[211] = sizes[7]                              # exact duplicates, far apart in the table
    sizes[12] = sizes[11]                              # ... and adjacent
    data["chair"] = [_entry("chair", k, sizes[k], lo=rng.uniform(-1, 1, size=3)) for k in range(300)]
    data["chair"][211]["bbox_min"], data["chair"][211]["bbox_max"] = list(data["chair"][7]["bbox_min"]), list(data["chair"][7]["bbox_max"])
    data["chair"][12]["bbox_min"], data["chair"][12]["bbox_max"] = list(data["chair"][11]["bbox_min"]), list(data["chair"][11]["bbox_max"])
    data["desk"] = [_entry("desk", 0, (1.4, 0.75, 0.7))]
    data["lamp"] = []
    s = rng.uniform(0.5, 1.5, size=(6, 3))
    data["sofa"] = [_entry("sofa", k, s[k // 2]) for k in range(6)]                  # three pairs of duplicates
    data["slab"] = [_entry("slab", 0, (1.0, 0.2, 1.0)), _entry("slab", 1, (0.5, 0.5, 0.5)), _entry("slab", 2, (0.0, 0.4, 0.9)),
                    _entry("slab", 3, (0.0, 1.0, 1.0)), _entry("slab", 4, (1.0, 1.0, 1.0))]
    # last-bit pairs: bbox_min 0 and x size 1, so the ratios ARE the y / z sizes; neighbours one float64 step apart, in both orders
    shelf, k = [], 0
    for y, z in rng.uniform(0.4, 1.8, size=(8, 2)):
        up = (np.nextafter(y, 2.0), z) if k % 4 < 2 else (y, np.nextafter(z, 2.0))
        pair = [(y, z), up] if k % 2 == 0 else [up, (y, z)]
        for yy, zz in pair:
            shelf.append(_entry("shelf", len(shelf), (1.0, yy, zz)))
        k += 1
    data["shelf"] = shelf
    # wall table: 40 entries, duplicates (3 == 17, 20 == 21) and a last-bit pair (30, 31)
    W = 40
    ws, fs = rng.uniform(2.0, 8.0, size=(W, 3)), rng.uniform(2.0, 8.0, size=(W, 3))
    wlo, flo = rng.uniform(-3, 3, size=(W, 3)), rng.uniform(-3, 3, size=(W, 3))
    ws[30], fs[30] = (1.0, 0.61, 1.27), (1.0, 0.1, 1.27)
    ws[31], fs[31] = (1.0, 0.61, np.nextafter(1.27, 2.0)), (1.0, 0.1, np.nextafter(1.27, 2.0))
    wlo[30:32], flo[30:32] = 0.0, 0.0                  # (so that max - min IS the size, to the bit)
    wall = [{"house_id": "h%02d" % j, "model_id": "m%02d" % j, "wall_bbox_min": [float(x) for x in wlo[j]],
             "wall_bbox_max": [float(x) for x in wlo[j] + ws[j]], "floor_bbox_min": [float(x) for x in flo[j]],
             "floor_bbox_max": [float(x) for x in flo[j] + fs[j]]} for j in range(W)]
    for dup, of in ((17, 3), (21, 20)):
        for k in ("wall_bbox_min", "wall_bbox_max", "floor_bbox_min", "floor_bbox_max"):
            wall[dup][k] = list(wall[of][k])
    return data, wall


def rooms(rng):
    """[(objs int list, boxes float32 [n, 6])] with the room row last"""
    out = []

    def box(n):
        lo = rng.uniform(0.0, 0.6, size=(n, 3))
        return np.concatenate([lo, lo + rng.uniform(0.05, 0.4, size=(n, 3))], 1).astype(np.float32)

    def room(ext):
        return np.array([[0, 0, 0, ext[0], ext[1], ext[2]]], dtype=np.float32)

    with_models = [1, 2, 3, 5, 6, 7]
    for r in range(36):
        n = int(rng.integers(1, 14))
        objs = [int(x) for x in rng.choice(with_models, size=n, p=[0.1, 0.45, 0.05, 0.1, 0.1, 0.2])]
        out.append((objs + [0], np.concatenate([box(n), room(rng.uniform(2.5, 7.0, size=3))])))
    # a room of the shelf's own ratios: boxes whose (y/x, z/x) fall next to the last-bit pairs
    b = box(12)
    out.append(([7] * 12 + [0], np.concatenate([b, room((3.0, 3.0, 3.0))])))
    # the wall table's last-bit pair: a room of its very ratio
    out.append(([2, 0], np.concatenate([box(1), room((2.0, 1.22, 2.54))])))
    # zero-width boxes: slab (NaN against the zero-width models: the first of them wins), chair (all-infinite: index 0), and a box of zero
    # width AND height (0 / 0: every distance NaN, index 0); a regular slab row next to them
    z = box(6)
    z[0, 3] = z[0, 0]; z[1, 3] = z[1, 0]; z[2, 3] = z[2, 0]; z[2, 4] = z[2, 1]; z[3, 3] = z[3, 0]; z[3, 4] = z[3, 1]; z[5, 3] = z[5, 0]
    out.append(([6, 2, 6, 2, 6, 6, 0], np.concatenate([z, room((4.0, 2.7, 5.0))])))
    # a class without models (lamp) next to classes with
    out.append(([2, 4, 1, 4, 0], np.concatenate([box(4), room((5.0, 2.5, 3.0))])))
    return out


def reference_namespace(data, wall):
    ns = dict(np=_numpy_namespace(), suncg_data=data, object_idx_to_name=list(VOCAB), wall_data_json=wall)
    names = ["suncg_retrieve", "wall_retrieve", "floor_retrieve"]
    nodes = _top_level(SRC, names)
    _run([nodes[n] for n in names], ns, SRC)
    return ns


def write_npz(path, arrays):
    """np.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    RT = importlib.import_module("3d_sln_amd.host.retrieve")
    rng = np.random.default_rng(20260)
    data, wall = tables(rng)
    rms = rooms(rng)
    ns = reference_namespace(data, wall)
    warnings.simplefilter("ignore", RuntimeWarning)           # the zero-width rows divide by zero on purpose

    def copies(boxes):
        return [torch.from_numpy(b.copy()) for b in boxes]

    index_of = {name: {e["id"]: k for k, e in enumerate(v)} for name, v in data.items()}
    objs_all, boxes_all, room_row, choice, wall_choice, floor_choice, last_row = [], [], [], [], [], [], []
    row0 = 0
    for objs, boxes in rms:
        n = len(objs)
        empty = [i for i, c in enumerate(objs[:-1]) if len(data[VOCAB[c]]) == 0]
        if empty:
            try:
                ns["suncg_retrieve"](list(objs), copies(boxes))
            except ValueError:
                pass
            else:
                raise AssertionError("the reference did not raise on a class without models")
        keep = [i for i in range(n) if i not in empty]
        ids = ns["suncg_retrieve"]([objs[i] for i in keep], copies(boxes[keep]))
        assert len(ids) == len(keep) - 1
        ch = [-1] * n
        for i, mid in zip(keep[:-1], ids):
            # an id names one table entry; duplicates of a bounding box have ids of their own
            ch[i] = index_of[VOCAB[objs[i]]][mid]
        w, f = ns["wall_retrieve"](copies(boxes)), ns["floor_retrieve"](copies(boxes))
        wall_choice.append(next(j for j, e in enumerate(wall) if e is w))
        floor_choice.append(next(j for j, e in enumerate(wall) if e is f))
        objs_all += objs; boxes_all.append(boxes); choice += ch
        room_row += [row0 + n - 1] * n; last_row.append(row0 + n - 1); row0 += n
    boxes_all = np.concatenate(boxes_all).astype(np.float32)
    M = sum(len(data[c]) for c in VOCAB[1:])
    out = dict(objs=np.asarray(objs_all, np.int32), boxes=boxes_all, room_row=np.asarray(room_row, np.int32), choice=np.asarray(choice, np.int32),
               last_row=np.asarray(last_row, np.int32), wall_choice=np.asarray(wall_choice, np.int32), floor_choice=np.asarray(floor_choice, np.int32),
               vocab=np.frombuffer("\n".join(VOCAB).encode(), dtype=np.uint8),
               model_class=np.asarray([ci for ci, c in enumerate(VOCAB) for _ in data.get(c, [])], np.int32),
               model_ids=np.frombuffer("\n".join(e["id"] for c in VOCAB for e in data.get(c, [])).encode(), dtype=np.uint8),
               model_bbox=np.asarray([[e["bbox_min"], e["bbox_max"]] for c in VOCAB for e in data.get(c, [])], np.float64),
               wall_bbox=np.asarray([[e["wall_bbox_min"], e["wall_bbox_max"]] for e in wall], np.float64),
               floor_bbox=np.asarray([[e["floor_bbox_min"], e["floor_bbox_max"]] for e in wall], np.float64))
    assert out["model_bbox"].shape == (M, 2, 3)
    # what the fixture covers, stated and asserted
    ch, ob = out["choice"], out["objs"]
    counts = sorted(set(len(data.get(c, [])) for c in VOCAB[1:]))
    assert counts[:3] == [0, 1, 2] and 300 in counts, counts
    assert ((ob == 2) & (ch == 7)).any() or ((ob == 2) & (ch == 11)).any() or (ob == 5).any()
    assert not ((ob == 2) & ((ch == 211) | (ch == 12))).any() and not ((ob == 5) & (ch % 2 == 1)).any(), "a duplicate's second copy won"
    assert ((ob == 6) & (ch == 2)).sum() >= 2 and ((ob == 4) & (ch == -1)).sum() == 2
    shelf_rows = np.nonzero(ob == 7)[0]
    assert len(set(ch[shelf_rows] // 2)) >= 3 and len(set(ch[shelf_rows] % 2)) == 2, "the last-bit pairs are not exercised on both sides"
    # the restatement against what the reference chose: 0 differing rows
    table = RT.ModelTable(data, VOCAB)
    got = RT.retrieve_models_torch(torch.from_numpy(boxes_all), torch.from_numpy(out["objs"]), torch.from_numpy(out["room_row"]), table).numpy()
    wr, fr = RT.shell_ratios(wall)
    sh = RT.retrieve_shell_torch(torch.from_numpy(boxes_all), torch.from_numpy(out["last_row"]), torch.from_numpy(wr), torch.from_numpy(fr)).numpy()
    diffs = dict(models=int((got != ch).sum()), wall=int((sh[:, 0] != out["wall_choice"]).sum()), floor=int((sh[:, 1] != out["floor_choice"]).sum()))
    print("rows %d (rooms %d), models %d, walls %d: differing %s" % (len(ch), len(rms), M, len(wall), diffs))
    assert not any(diffs.values()), diffs
    path = os.path.join(GOLD, "mesh_retrieve.npz")
    write_npz(path, out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
