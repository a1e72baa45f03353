"""Golden fixture for the refinement pictures (host/scene_pictures.py), produced by EXECUTING THE REFERENCE'S OWN SOURCE TEXT (needs the
reference tree; build container only).

``save_images`` (testing/test_render_refine.py:144-163), ``save_label_depth`` (:118-142), ``save_label`` (:165-190), ``nyu_class`` (:32),
``mapped_colors`` (:34-76) and the two label statements of ``finetune_VAE`` (:343-344) are taken out of the source text with ``ast`` and
``exec``ed unmodified.

What is injected (and therefore NOT pinned by this fixture): a recording ``imageio`` namespace - ``get_writer(path, mode)`` returns an
object whose ``append_data`` keeps the array (imageio is not installed; what it would encode is exactly that array).  The label
statements see ``target_labels_pooled = [image[:, 1:41]]``: the full-resolution planes instead of the pooled ones.

Inputs: tests/scene_picture_cases.py (our own code).  Recorded per case and room: the depth picture, the 40 masks of
``save_semantic=True`` on the 41-channel slice (on 70 channels the reference raises IndexError at ``nyu_class[40]``), ``flat_target`` of
the label statements, ``save_label``'s 40 + 1 masks, and for the one 256 x 256 case (``save_label_depth`` hard-codes its canvas) the
class-colour picture and its depth picture.  Before writing the tool asserts that ``scene_pictures_torch`` reproduces every recorded
array with 0 differing bytes, that every case stays inside the domain (planes in [0, 1], no d == 10, m > 0), and that ``save_label``'s
masks are 255 * (labels == 1 + c) and 255 * (labels == 0).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_scene_pictures.py

Writes tests/golden/scene_pictures.npz (numeric arrays only).
"""
import ast
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
from oracle.gen_golden_refine import GOLD, REF, _run, _top_level      # noqa: E402

SRC = os.path.join(REF, "testing/test_render_refine.py")
LABEL_LINES = (343, 344)


class _Writer:
    def __init__(self, log, path, mode):
        self.log, self.path, self.mode = log, path, mode

    def append_data(self, a):
        self.log.append((os.path.basename(self.path), self.mode, np.array(a, copy=True)))

    def close(self):
        pass


def reference_namespace(log):
    imageio = types.SimpleNamespace(get_writer=lambda path, mode=None: _Writer(log, path, mode))
    ns = dict(os=os, np=np, torch=torch, imageio=imageio)
    names = ["nyu_class", "mapped_colors", "save_label_depth", "save_images", "save_label", "finetune_VAE"]
    nodes = _top_level(SRC, names)
    _run([nodes[n] for n in names[:-1]], ns, SRC)
    stmts = sorted((n for n in ast.walk(nodes["finetune_VAE"]) if isinstance(n, ast.Assign) and n.lineno in LABEL_LINES), key=lambda n: n.lineno)
    assert [n.lineno for n in stmts] == list(LABEL_LINES) and "argmax" in ast.unparse(stmts[0]) and "-100" in ast.unparse(stmts[1])
    label_code = compile(ast.Module(body=stmts, type_ignores=[]), SRC, "exec")

    def flat_target(planes):
        loc = dict(torch=torch, target_labels_pooled=[planes], pooled_idx=0)
        exec(label_code, loc)
        return loc["flat_target"]

    ns["_flat_target"] = flat_target
    return ns


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    K = importlib.import_module("scene_picture_cases")
    SP = importlib.import_module("3d_sln_amd.host.scene_pictures")
    log = []
    ns = reference_namespace(log)
    tmp = tempfile.mkdtemp()
    out = {}

    def ran(fn, *a, **k):
        del log[:]
        fn(*a, folder_name=tmp, prefix="p", **k)
        return {name: arr for name, _, arr in log}

    for name in K.FIXTURE_CASES:
        img = K.case(name)
        assert K.in_domain(img), name
        t = torch.from_numpy(img.copy())
        B, C, S, _ = img.shape
        rec = dict(depth=[], masks=[], flat=[], color=[])
        for b in range(B):
            room = t[b:b + 1]
            got = ran(ns["save_images"], room[:, :41], save_semantic=True)
            plain = ran(ns["save_images"], room)                                   # the call of :320 / :377
            assert sorted(got) == sorted(["p_depth.gif"] + ["p_%s.gif" % n for n in ns["nyu_class"]]) and list(plain) == ["p_depth.gif"]
            assert np.array_equal(plain["p_depth.gif"], got["p_depth.gif"])
            rec["depth"].append(got["p_depth.gif"])
            rec["masks"].append(np.stack([got["p_%s.gif" % n] for n in ns["nyu_class"]]))
            flat = ns["_flat_target"](room[:, 1:41])                               # [1, 1, S, S] int64: class 0..39, -100 where empty
            rec["flat"].append(flat[0, 0].numpy().astype(np.int16))
            lab = ran(ns["save_label"], flat.float())
            labels = np.where(rec["flat"][-1] < 0, 0, rec["flat"][-1] + 1)
            for c, n in enumerate(ns["nyu_class"]):
                assert np.array_equal(lab["p_%s.gif" % n], 255 * (labels == 1 + c)), (name, n)
            assert np.array_equal(lab["p_empty_class.gif"], 255 * (labels == 0)), name
            if S == 256:
                ld = ran(ns["save_label_depth"], flat.float(), room[:, :1])
                assert np.array_equal(ld["p_depth.png"], got["p_depth.gif"])
                rec["color"].append(ld["p_class_color.png"])
        rec = {k: np.stack(v) for k, v in rec.items() if v}
        for k, v in rec.items():
            assert v.dtype == (np.int16 if k == "flat" else np.uint8), (k, v.dtype)
        # the restatement against what the reference wrote: 0 differing bytes
        pics = SP.scene_pictures_torch(t)
        want_labels = np.where(rec["flat"] < 0, 0, rec["flat"] + 1).astype(np.uint8)
        diffs = dict(depth=int((pics.depth8.numpy() != rec["depth"]).sum()), masks=int((pics.masks8.numpy() != rec["masks"]).sum()),
                     labels=int((pics.labels.numpy() != want_labels).sum()), status=int(pics.status.abs().sum()))
        if "color" in rec:
            diffs["color"] = int((pics.rgb.numpy() != rec["color"]).sum())
        print("%-12s %s: differing bytes %s; classes %d, empty %.1f %%" % (name, img.shape, diffs, len(np.unique(want_labels)) - 1, 100 * (want_labels == 0).mean()))
        assert not any(diffs.values()), (name, diffs)
        out[name + ":sha256"] = np.frombuffer(K.sha256(img).encode(), dtype=np.uint8)
        for k, v in rec.items():
            out["%s:%s" % (name, k)] = v
    out["cases"] = np.frombuffer(",".join(K.FIXTURE_CASES).encode(), dtype=np.uint8)
    out["palette"] = np.asarray(ns["mapped_colors"], np.uint8)
    out["class_names"] = np.frombuffer("\n".join(ns["nyu_class"]).encode(), dtype=np.uint8)
    assert out["palette"].shape == (41, 3) and len(ns["nyu_class"]) == 40
    path = os.path.join(GOLD, "scene_pictures.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == "__main__":
    main()
