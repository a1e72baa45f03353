"""The refinement pictures (host/scene_pictures.py) on the CPU: the torch restatement against the executed reference
(tests/golden/scene_pictures.npz, tools/gen_golden_scene_pictures.py), the palette and class names, the class-index encoding shared with
host/spade_input.py, the argument checks that need no device, and the C ABI's new symbols."""
import os
import re

import numpy as np
import pytest
import torch

import scene_picture_cases as K
from conftest import ROOT, load_golden, pkg


def SP():
    return pkg("host.scene_pictures")


def _labels_of(flat):
    """:343-344's flat_target (class 0..39, -100 where empty) as the class-index image"""
    return np.where(flat < 0, 0, flat + 1).astype(np.uint8)


def test_restatement_equals_the_executed_reference():
    g = load_golden("scene_pictures")
    names = bytes(g["cases"]).decode().split(",")
    assert tuple(names) == K.FIXTURE_CASES
    sizes = set()
    for name in names:
        img = K.case(name)
        assert K.sha256(img) == bytes(g[name + ":sha256"]).decode(), "the inputs of %s are not the fixture's" % name
        assert K.in_domain(img)
        sizes.add(img.shape[-1])
        pics = SP().scene_pictures_torch(torch.from_numpy(img.copy()))
        want = dict(depth8=g[name + ":depth"], masks8=g[name + ":masks"], labels=_labels_of(g[name + ":flat"]))
        if name + ":color" in g.files:
            want["rgb"] = g[name + ":color"]
        for k, w in want.items():
            got = getattr(pics, k).numpy()
            assert got.dtype == np.uint8 and got.shape == w.shape, (name, k, got.shape, w.shape)
            assert int((got != w).sum()) == 0, "%s %s: %d differing bytes" % (name, k, int((got != w).sum()))
        assert pics.status.tolist() == [0] * img.shape[0]
        # rgb of every case: the palette the reference's source holds, looked up with the recorded labels
        assert np.array_equal(pics.rgb.numpy(), g["palette"][want["labels"]])
    assert sizes == {4, 12, 64, 256}
    assert sum(1 for n in names if n + ":color" in g.files) == 1          # save_label_depth hard-codes its canvas


def test_the_fixture_cases_hold_what_they_are_for():
    g = load_golden("scene_pictures")
    # S = 64: four workgroups a room; the minimum in the last one only, the maximum below 10 in workgroup b, both differ per room
    img = K.case("s64_b3_c41")
    n = K.PX_PER_GROUP
    mins, maxs = [], []
    for b, room in enumerate(img):
        d = room[0].reshape(-1)
        assert d.size // n == 4 and int(d.argmin()) // n == 3 and float(d[:3 * n].min()) > float(d.min())
        e = d - d.min()
        m = e[e < 10].max()
        where = np.flatnonzero(e == m) // n
        assert set(where.tolist()) == {b} and float(np.sort(np.unique(e[e < 10]))[-2]) <= m - 0.5
        assert bool((e > 10).any())
        mins.append(float(d.min())); maxs.append(float(m))
    assert len(set(mins)) == 3 and len(set(maxs)) == 3
    # ties, the two sums around 0.5, the background, values above min + 10
    for name in K.FIXTURE_CASES:
        img = K.case(name)
        sem = img[:, 1:41]
        s = sem.sum(1)
        assert bool(((sem == 1).sum(1) == 2).any()), name
        assert bool((s == 0.5).any()) and bool((s == 0.49609375).any()), name
        lab = _labels_of(g[name + ":flat"])
        assert bool((lab[s == 0.5] > 0).all()) and bool((lab[s == 0.49609375] == 0).all())
        assert float(img[:, 0].min()) <= -1.0


def test_palette_and_class_names_are_the_references():
    g = load_golden("scene_pictures")
    S, P = SP(), pkg("host.plot2d")
    assert np.array_equal(np.asarray(S.CLASS_COLORS, np.uint8), g["palette"])
    assert S.CLASS_COLORS == ((0, 0, 0),) + tuple(P.MAPPED_COLORS)
    assert list(S.NYU_CLASS) == bytes(g["class_names"]).decode().split("\n")
    pal = S.palette_tensor()
    assert pal.dtype == torch.int32 and pal.tolist() == [r | gg << 8 | b << 16 for r, gg, b in S.CLASS_COLORS]


def test_labels_are_the_class_index_image_of_spade_input():
    I = pkg("host.spade_input")
    g = load_golden("scene_pictures")
    img = K.case("s12_c70")
    pics = SP().scene_pictures_torch(torch.from_numpy(img.copy()))
    labels = pics.labels[0]
    masks = I.masks_from_labels(labels)
    present = sorted(set(labels.flatten().tolist()) - {0})
    assert sorted(masks) == sorted(I.NYU40[c - 1] for c in present) and len(present) >= 4
    assert torch.equal(I.labels_from_masks(masks, labels.shape), labels)
    for c in present:                                                     # save_label's masks: 255 where the class wins
        assert np.array_equal(masks[I.NYU40[c - 1]].numpy(), 255 * (_labels_of(g["s12_c70:flat"])[0] == c))


def test_live_flags_in_the_restatement():
    dirty, live, clean = K.live_case()
    sem = live[:, 1:41]
    assert bool(((sem & 1) == 0).any()) and bool((sem == 1).any()) and bool((live[:, 41:] == 1).any()) and bool(np.isnan(dirty).any())
    S = SP()
    a = S.scene_pictures_torch(torch.from_numpy(dirty), torch.from_numpy(live))
    b = S.scene_pictures_torch(torch.from_numpy(clean))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_status_in_the_restatement():
    pics = SP().scene_pictures_torch(torch.from_numpy(K.status_case()))
    assert pics.status.tolist() == [0, 1, 2, 0]
    assert int(pics.depth8[1].max()) == 0 and int(pics.depth8[2].max()) == 0
    assert int(pics.depth8[0].max()) == 255 and int(pics.depth8[3].max()) == 255 and not torch.equal(pics.depth8[0], pics.depth8[3])
    assert torch.equal(pics.labels[1], pics.labels[0]) and torch.equal(pics.labels[2], pics.labels[0])


@pytest.mark.parametrize("kw", [dict(S=6), dict(S=0), dict(S=8, batch=0), dict(S=8, channels=42), dict(S=8, channels=40)])
def test_scene_pictures_refuses_a_geometry_the_kernel_does_not_take(kw):
    with pytest.raises(ValueError):
        SP().ScenePictures(device="cuda", **kw)                           # refused before the device is touched


def test_scene_pictures_has_no_cpu_path():
    L = pkg("_lib")
    with pytest.raises(L.SlnError):
        SP().ScenePictures(8, device="cpu")


def test_new_symbols_are_declared_and_bound():
    L = pkg("_lib")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sln_hip.h")).read(), flags=re.S)
    for name in ("sln_scene_pictures_workspace_bytes", "sln_scene_pictures"):
        assert re.search(r"\b%s\s*\(" % name, txt) and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert len(L.SIGNATURES["sln_scene_pictures"][1]) == 13
    lib = L.lib()
    # the size and argument rules need no device: nothing is launched for them
    assert lib.sln_scene_pictures_workspace_bytes(3, 64) == 3 * 4 * 2 * 4
    assert lib.sln_scene_pictures_workspace_bytes(1, 4) == 8
    assert lib.sln_scene_pictures_workspace_bytes(1, 6) == -2 and lib.sln_scene_pictures_workspace_bytes(0, 8) == -1
    for B, C, S in ((1, 41, 6), (0, 41, 8), (1, 42, 8)):
        assert lib.sln_scene_pictures(None, B, C, S, None, None, None, None, None, None, None, None, None) == -2
    assert lib.sln_scene_pictures(None, 1, 41, 8, None, None, None, None, None, None, None, None, None) == -1
