"""host/observe.py on the CPU: ``observed_target_torch`` (the yardstick of the kernel tests) against a pixel-by-pixel restatement in Python
ints and numpy scalars, the status bits of the hand-made cases, and a round trip through the CPU oracle: render a room, observe the
render (plane 0 + the scene_pictures labels), rebuild the target from the observation, compare with the render."""
import os
import re

import numpy as np
import pytest
import torch

import observed_cases as OC
from conftest import ROOT, load_golden, pkg
from oracle import refine_ref as rf

CASES = OC.cases()
SMALL = [c for c in CASES if c["depth"].shape[-1] <= 12]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_torch_definition_equals_the_python_loop_restatement(case):
    OB = pkg("host.observe")
    got, status = OB.observed_target_torch(case["depth"], case["labels"], OC.CHAN, OC.DCH, OC.NCH)
    want, want_status = OC.loop_restatement(case["depth"], case["labels"])
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.equal(_bits(got), _bits(torch.from_numpy(want))), "planes that differ: %s" % sorted(
        set(torch.nonzero(_bits(got) != _bits(torch.from_numpy(want)))[:, 1].tolist()))
    assert status.tolist() == want_status


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_status_bits_and_exact_planes_of_the_cases(case):
    OB = pkg("host.observe")
    got, status = OB.observed_target_torch(case["depth"], case["labels"], OC.CHAN, OC.DCH, OC.NCH)
    if case["status"] is not None:
        assert status.tolist() == case["status"]
    for room, plane in case["ones"]:
        assert bool((got[room, plane] == 1.0).all()), "plane %d of room %d is not exactly 1.0" % (plane, room)
    sem = got[:, 1:41]
    assert bool(((sem == 0.0) | (sem == 1.0)).all()) and bool((sem.sum(1) <= 1.0).all())
    d0 = got[:, 0]
    assert bool(((d0 == -1.0) | ((d0 > 0) & (d0 <= 15.0))).all())
    assert bool(torch.isfinite(got).all())
    # a labelled pixel of the target is a pixel with a reading, labelled by a byte <= 40
    lab = case["labels"].long()
    keep = (lab <= 40) & (case["depth"] > 0) & (case["depth"] <= 15)
    assert torch.equal(sem.argmax(1)[sem.sum(1) > 0] + 1, lab[keep & (lab > 0)])


def test_largest_sum_stays_exact():
    """96 x 96 pixels at depth 15: the mean of the fixed-point sum is 15 again, the depth-hot plane 15 / 10"""
    OB = pkg("host.observe")
    case = [c for c in CASES if c["name"] == "largest_sum_s96"][0]
    got, _ = OB.observed_target_torch(case["depth"], case["labels"], OC.CHAN, OC.DCH, OC.NCH)
    plane = got[0, OC.plane_of(4)]
    assert bool((plane == np.float32(15.0) / np.float32(10.0)).all())


def test_refused_tables_and_inputs():
    OB = pkg("host.observe")
    d, l = CASES[0]["depth"], CASES[0]["labels"]
    with pytest.raises(ValueError):
        OB.observed_target_torch(d, l, OC.CHAN, OC.DCH, 69)
    with pytest.raises(ValueError):
        OB.observed_target_torch(d, l, [40] + OC.CHAN[1:], OC.DCH, 70)
    with pytest.raises(ValueError):
        OB.observed_target_torch(d, l, OC.CHAN, OC.DCH[:-1] + [OC.DCH[-2]], 70)
    with pytest.raises(ValueError):
        OB.observed_target_torch(d, l.float(), OC.CHAN, OC.DCH, 70)
    with pytest.raises(ValueError):
        OB.observe(torch.zeros(1, 3, 4, 4))


def test_entry_point_is_declared_mirrored_and_built_without_contraction():
    L = pkg("_lib"); B = pkg("build")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sln_hip.h")).read(), flags=re.S)
    for name in ("sln_observed_target_workspace_bytes", "sln_observed_target"):
        assert re.search(r"\b%s\s*\(" % name, txt) and name in L.SIGNATURES
    assert len(L.SIGNATURES["sln_observed_target"][1]) == 12
    assert "-ffp-contract=off" in B.PER_FILE["observed_target.hip"] and "observed_target.hip" in B.sources()


@pytest.mark.parametrize("tag,S", [("s64", 64), ("s256", 256)])
def test_round_trip_through_the_cpu_oracle(tag, S):
    """render_room -> observe -> observed_target_torch against the render.  Plane 0: equal.  Semantic planes: within 32 * 2^-24 (the
    render's value is a trilinear sum of eight three-factor weights plus class_image_value, ~17 roundings; the rebuilt planes are
    exactly 0 or 1).  Depth-hot planes: within 2^-23 (the oracle averages in fp32, the definition in fixed point: one ulp at values <= 1)."""
    OB = pkg("host.observe"); DR = pkg("host.diff_render"); SP = pkg("host.scene_pictures")
    g = load_golden("refine_scene")
    tables = rf.load_tables(g)
    p = tag + ":"
    names = [(["__room__"] + rf.FIXTURE_VOCAB)[int(o)] for o in g[p + "objs"]]
    with torch.no_grad():
        render, _, _ = rf.render_room(torch.from_numpy(g[p + "boxes"]), torch.from_numpy(g[p + "angles"]).float(), names, tables, S)
    _, chan, dch = DR.class_tables(list(tables["vocab"]) + ["ceiling", "floor", "wall"])
    depth, labels = OB.observe(render)
    assert depth.dtype == torch.float32 and labels.dtype == torch.uint8 and tuple(labels.shape) == (1, S, S)
    # the precondition of everything below: no class pixel lacks a reading and no reading lacks a class
    reading = (depth > 0) & (depth <= 15)
    assert torch.equal(reading, labels > 0)
    target, status = OB.observed_target_torch(depth, labels, chan, dch)
    assert status.tolist() == [0]
    assert torch.equal(target[:, 0], render[:, 0])
    sem = float((target[:, 1:41] - render[:, 1:41]).abs().max())
    hot = float((target[:, 41:] - render[:, 41:]).abs().max())
    print("%s: semantic planes max |diff| = %.3g (%.1f x 2^-24), depth-hot planes max |diff| = %.3g, %d elements in %d planes differ" % (
        tag, sem, sem * 2 ** 24, hot, int((target[:, 41:] != render[:, 41:]).sum()),
        int((target[:, 41:] != render[:, 41:]).flatten(2).any(2).sum())))
    assert sem <= 32 * 2.0 ** -24
    assert hot <= 2.0 ** -23
    assert torch.equal(SP.scene_pictures_torch(target, masks=False).labels, labels)
