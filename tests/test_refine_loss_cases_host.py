"""The operands of tests/refine_loss_cases.py meet what lets test_refine_loss_family_gpu.py compare EVERY element (CPU only, from the
reference alone): no pooled depth difference, depth sum or label decision sits close enough to its threshold for fp32 rounding to move it.
Also the route table - which pooling and which backward kernel a geometry takes, from the host-side tables with the launchers' own
rules - and the refusals of the entry points that return before anything is launched."""
import ctypes as C

import pytest
import torch

from conftest import pkg

import refine_loss_cases as RC

F64, F32 = torch.float64, torch.float32


@pytest.mark.parametrize("name", RC.NAMES)
def test_operands_keep_every_decision_away_from_its_threshold(name):
    c, ops = RC.BY_NAME[name], RC.operands(name)
    sizes, nd = c["sizes"], c["C"] - 41
    image, target = ops["image"].double(), RC.clean_target(ops).double()
    labels, vp = RC.masked_labels(name)
    # depth sums: the null decision (sum < 0.5) of every pixel, and the null block is what it says
    dsum = image[:, 41:].sum(1)
    assert float((dsum - 0.5).abs().min()) >= 0.05
    assert torch.equal(dsum < 0.5, ops["null"]) and bool(ops["null"].any()) and not bool(ops["null"].all())
    # pooled depth differences over the compared elements: the plane's sign, nowhere closer to 0 than 1e-3 (0.05 by construction)
    diff = RC.pooled(image, sizes, 1, F64)[:, :, 40:] - RC.pooled(target, sizes, 0, F64)[:, :, 40:]
    sign = ops["sign"][:, None, :, None, None].expand_as(diff)
    keep = torch.ones_like(diff, dtype=torch.bool) if vp is None else vp[:, :, None].expand_as(diff)
    if not RC.is_all_invalid(c):
        assert float(diff.abs()[keep].min()) >= 1e-3
        assert bool((torch.sign(diff) == sign)[keep].all())
        assert bool((ops["sign"][:, :-1] < 0).any()) and bool((ops["sign"] > 0).any())
    # labels: margins of the argmax and of the "nothing here" rule on the pooled one-hot block; fp32 decides the same
    sem = RC.pooled(target, sizes, 0, F64)[:, :, :40]
    total = sem.sum(2)
    top = sem.topk(2, dim=2).values
    assert float((total - 0.5).abs().min()) >= 1e-3
    if not RC.is_all_invalid(c):                                  # (its cleaned target is all zeros: nothing to decide)
        assert float((top[:, :, 0] - top[:, :, 1])[total >= 0.5].min()) >= 1e-4
    lab32 = RC.labels_of(RC.clean_target(ops), sizes, F32)
    assert torch.equal(lab32, RC.labels_of(RC.clean_target(ops), sizes, F64))
    assert bool((lab32 == -100).any()) and (RC.is_all_invalid(c) or len(torch.unique(lab32)) > 3)
    # the mask: every room keeps a valid pooled pixel and a label per scale (the all-invalid case keeps none)
    if vp is not None:
        kept = (labels >= 0).sum(dim=(2, 3))
        if RC.is_all_invalid(c):
            assert int(vp.sum()) == 0 and int(kept.sum()) == 0
        else:
            assert bool((vp.sum(dim=(1, 2, 3)) > 0).all()) and bool((kept > 0).all())
            assert not bool(vp.all()), "the mask removes no pooled pixel"
        assert bool(torch.isnan(ops["target"]).any()) == bool((ops["valid"] == 0).any())
    assert image.shape[1] - 41 == nd and torch.isfinite(ops["image"]).all()


@pytest.mark.parametrize("geometry", sorted(RC.GEOMETRIES))
def test_route_table(geometry):
    """A change of the table builder or of a case that moves a geometry to another kernel fails here, not silently."""
    g = RC.GEOMETRIES[geometry]
    stride, P, max_col, pool, backward = RC.host_tables(g["S"], g["sizes"])
    assert (stride, P) == (max(g["sizes"]), g["sizes"][-1])
    assert pool == g["pool"], (pool, stride, P)
    assert max_col == g["max_col"] and backward == g["backward"], (max_col, backward)
    # the two refusals that depend on the geometry alone
    assert ((P * P) % 128 == 0) == g["report"]
    assert ((len(g["sizes"]) * P * P) % 128 == 0) == g["rooms_ok"]


def test_edges_the_family_has_to_reach_are_in_the_case_list():
    G = RC.GEOMETRIES
    assert G["s40_3scales"]["S"] % 16 == 8 and len(G["s40_3scales"]["sizes"]) == 3                 # last strip of 8 rows, fewer than 4 scales
    assert G["s264_2blocks"]["S"] > 256 and G["s264_2blocks"]["S"] % 16 == 8                       # second column block, 8 active lanes
    assert max(G["s24_upsample"]["sizes"]) > RC.POOL_LDS_MAX >= G["s24_upsample"]["sizes"][-1]     # pool_kernel by the stride
    assert G["s40_p104"]["sizes"][-1] > RC.POOL_LDS_MAX                                            # ... and by the pooled size
    assert G["s40_generic"]["sizes"][-1] <= RC.SEP_MAX_P and G["s40_generic"]["max_col"] > RC.SEP_MAX_ENTRIES      # generic backward by geometry
    assert (G["s36_tail"]["sizes"][-1] ** 2) % 128 != 0 and (3 * G["s36_tail"]["sizes"][-1] ** 2) % 128 != 0     # tail block of loss_kernel
    assert G["s96_workload"]["max_col"] == RC.SEP_MAX_ENTRIES                                      # five entries in the register lists
    nd = {c["C"] - 41 for c in RC.CASES}
    assert nd == {29, 11} and 11 % 8 == 3                                                          # a DCH part of 3 and a last CG group of 3 (51 % 8)
    for g in G:
        cases = [c for c in RC.CASES if c["geometry"] == g]
        assert cases, g
        if g != "s96_workload" and g != "s264_2blocks":
            assert {c["B"] for c in cases} >= {1, 3}, g
            assert any(c["mask"] for c in cases) and any(not c["mask"] for c in cases), g
        if G[g]["rooms_ok"] and g != "s96_workload":
            assert any(c["per_room"] for c in cases), g


def _descriptor(L, geometry, B=1, per_room=0, C_=70):
    """a descriptor with host pointers in the table fields: enough for the checks that run before any launch"""
    g = RC.GEOMETRIES[geometry]
    d = L.SlnRefineLoss()
    d.B, d.image_size, d.pooled_size, d.channels = B, g["S"], g["sizes"][-1], C_
    d.sem0, d.n_sem, d.dep0, d.n_dep, d.n_scales, d.stage1_stride = 1, 40, 41, C_ - 41, len(g["sizes"]), max(g["sizes"])
    keep = torch.zeros(16, dtype=torch.int32)
    for f in ("s2_k0", "s2_k1", "s2_l1", "s1_i0", "s1_i1", "s1_l1", "col_ptr", "col_out", "col_w"):
        setattr(d, f, keep.data_ptr())
    d.max_col_entries, d.per_room = g["max_col"], per_room
    return d, keep


def test_refusals_of_the_loss_entry_points_before_any_launch():
    L = pkg("_lib")
    lib = L.lib()
    buf = torch.zeros(64)
    p = C.c_void_p(buf.data_ptr())
    # per_room where a 128-row block of loss_kernel would cover two rooms
    d, keep = _descriptor(L, "s36_tail", B=3, per_room=1)
    assert lib.sln_refine_loss_init(C.byref(d), p, None) == -2
    assert lib.sln_refine_loss_forward(C.byref(d), p, p, p, p, p, p, None) == -2 and lib.sln_refine_loss_backward(C.byref(d), p, p, p, None) == -2
    assert lib.sln_refine_loss_live_ok(C.byref(d)) == 0
    d.per_room = 0
    assert lib.sln_refine_loss_init(C.byref(d), p, None) == 0
    # the report needs whole 128-row blocks per (room, scale), and rooms
    for geometry, B, per_room, want in (("s40_p104", 1, 0, -2), ("s36_tail", 1, 0, -2), ("s40_3scales", 3, 0, -2)):
        d, keep = _descriptor(L, geometry, B=B, per_room=per_room)
        assert lib.sln_refine_report(C.byref(d), p, p, p, p, None, p, None) == want, geometry
    assert float(buf.abs().max()) == 0.0
    # live_planes: honoured on the LDS + separable route only
    for geometry, g in RC.GEOMETRIES.items():
        d, keep = _descriptor(L, geometry)
        assert lib.sln_refine_loss_live_ok(C.byref(d)) == int(g["pool"] == "lds" and g["backward"] == "separable"), geometry
    # a mask needs all three fields
    d, keep = _descriptor(L, "s40_3scales")
    d.valid_pooled = buf.data_ptr()
    assert lib.sln_refine_loss_init(C.byref(d), p, None) == -1


def test_refusals_of_the_update_launches_before_any_launch():
    """sln_refine_sgd_rooms / sln_refine_sgd: SLN_E_BADARG and nothing written for ranges that are no multiples of 4 floats, that leave the
    stride, for 0 and 97 ranges and for parameters that are not 16-byte aligned"""
    L = pkg("_lib")
    lib = L.lib()
    raw = torch.full((256 + 8,), 3.25)
    a0 = (-raw.data_ptr() // 4) % 4                              # first 16-byte aligned element
    p, g = raw[a0:a0 + 128], raw[a0 + 128:a0 + 256]
    assert p.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0
    z = torch.full((8,), 3.25)
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    i64 = lambda v: (C.c_int64 * len(v))(*v)

    def rooms(off, ln, n=None, stride=64, R=2, params=None):
        n = len(off) if n is None else n
        off, ln = off or [0], ln or [0]
        return lib.sln_refine_sgd_rooms(params or ptr(p), ptr(g), R, stride, i64(off), i64(ln), n, 0.5, ptr(z), ptr(z), 4, 0.5, None)
    assert rooms([0, 18], [8, 8]) == -1 and rooms([0, 16], [8, 6]) == -1                   # offset / length no multiple of 4
    assert rooms([0, 60], [8, 8]) == -1                                                    # off + len > stride
    assert rooms([], [], n=0) == -1 and rooms([0] * 97, [4] * 97) == -1                    # 0 and 97 ranges
    assert rooms([0], [8], params=ptr(p, 4)) == -1 and rooms([0], [8], stride=62) == -1    # misaligned parameters, stride
    assert rooms([0], [8], R=0) == -1
    assert lib.sln_refine_sgd(ptr(p, 4), ptr(g), 8, 0.5, ptr(z), ptr(z), 4, 0.5, None) == -1
    assert lib.sln_refine_sgd(ptr(p), ptr(g, 8), 8, 0.5, ptr(z), ptr(z), 4, 0.5, None) == -1
    assert lib.sln_refine_sgd(ptr(p), ptr(g), -1, 0.5, ptr(z), ptr(z), 4, 0.5, None) == -1
    assert lib.sln_refine_sgd(ptr(p), ptr(g), 8, 0.5, None, ptr(z), 4, 0.5, None) == -1
    assert lib.sln_refine_sgd(ptr(p), ptr(g), 0, 0.5, ptr(z), ptr(z), 0, 0.5, None) == 0   # nothing to do: no launch
    assert bool((raw == 3.25).all()) and bool((z == 3.25).all())
