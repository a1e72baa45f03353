"""The rasterizer's backward kernels per face against the double-sum reference (run with -m gpu): pixel_map_backward_kernel in its
dense, multi-pass and fused-scene policies, depth_backward_face_kernel and the two project_faces_bwd kernels.

Every element of a gradient is compared: |got - g64| <= raster_bwd_cases.sum_bound(S, n) with g64, S = sum |term| and n from the _f64
entry points of oracle/raster_ref.cpp, and exactly 0 where no term exists.  Cases and what each reaches: raster_bwd_cases.py,
test_raster_bwd_ref_host.py.  Operands go through raster_bwd_gpu_util.Operands: held until after the synchronisation, pairwise
distinct, every index map checked on the host (LAB_NOTES section 25)."""
import functools

import numpy as np
import pytest
import torch

import raster_bwd_cases as rc
import raster_bwd_gpu_util as ru
import raster_bwd_ref as rb
from gpu_util import SENT, _lib, _sync
from oracle import raster_ref as rr

pytestmark = pytest.mark.gpu

DENSE = {c.name: c for c in rc.DENSE}
MULTI = {c.name: c for c in rc.MULTI}
DEPTH = {c.name: c for c in rc.DEPTH}
SCENE = {c.name: c for c in rc.SCENE}


def _report(group, name, res):
    worst, where, nmax = res
    print("%s %s: worst err / allowed %.3f at %s, largest n %d" % (group, name, worst, where, nmax))


class _deterministic:
    """sln_set_deterministic(1) for the block, the earlier mode afterwards"""

    def __enter__(self):
        self.lib = _lib().lib()
        self.was = self.lib.sln_get_deterministic()
        self.lib.sln_set_deterministic(1)

    def __exit__(self, *exc):
        self.lib.sln_set_deterministic(self.was)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references: computed once per case, never written; kept only for the cases that more than one test uses
# ---------------------------------------------------------------------------------------------------------------------------------
DET = [("dense", "is65-g0"), ("dense", "B2-is130"), ("dense", "B9-is65"), ("multi", "P3-is65-B1"), ("depth", "is130"), ("depth", "B9-is65"),
       ("scene", "is65-B8")]
_KEPT = {}


def _shared(group):
    def deco(fn):
        @functools.wraps(fn)
        def get(name):
            if (group, name) in _KEPT:
                return _KEPT[(group, name)]
            v = fn(name)
            if (group, name) in DET:
                _KEPT[(group, name)] = v
            return v
        return get
    return deco


@_shared("dense")
def _dense(name):
    inp = rc.room_inputs() if name == "room" else rc.dense_inputs(DENSE[name])
    return inp, rr.nmr_backward_pixel_map_f64(*inp, rc.EPS)[:3]


@_shared("multi")
def _multi(name):
    inp = rc.multi_inputs(MULTI[name])
    return inp, rb.pixel_map_multi_f64(*inp, rc.EPS)[:3]


@_shared("depth")
def _depth(name):
    inp = rc.depth_inputs(DEPTH[name])
    return inp, rr.nmr_backward_depth_f64(*inp)


@_shared("scene")
def _scene(name):
    inp = rc.scene_inputs(SCENE[name])
    return inp, rb.scene_backward_f64(inp[0], inp[1], rc.SCENE_CHAN, rc.SCENE_DCH, inp[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_dense(faces, fi, rgb, grad, prefill=None):
    L = _lib()
    B, F = faces.shape[:2]
    is_, Cn = fi.shape[1], rgb.shape[-1]
    assert faces.shape == (B, F, 3, 3) and fi.shape == (B, is_, is_) and rgb.shape == grad.shape == (B, is_, is_, Cn)
    ru.check_index_map("face_index", fi, F)
    h = ru.Operands()
    for k, a in (("faces", faces), ("face_index", fi), ("rgb", rgb), ("grad_rgb", grad)):
        h.put(k, a)
    ru.guarded(h, "grad_faces", (B, F, 3, 3), prefill)
    h.launchable()
    L.check(L.lib().sln_raster_backward_rgb(h.p("faces"), h.p("face_index"), h.p("rgb"), h.p("grad_rgb"), B, F, is_, Cn, rc.EPS,
                                            h.p("grad_faces"), L.current_stream_ptr()), "backward_rgb")
    _sync("sln_raster_backward_rgb")
    return ru.read_guarded(h, "grad_faces", (B, F, 3, 3))


def _run_multi(faces, fi, passes, grads):
    L = _lib()
    B, F = faces.shape[:2]
    is_, P = fi.shape[1], len(passes)
    assert faces.shape == (B, F, 3, 3) and fi.shape == (B, is_, is_) and len(grads) == P
    assert all(a.shape == (B, 3, is_, is_) for a in list(passes) + list(grads))
    ru.check_index_map("face_index", fi, F)
    h = ru.Operands()
    h.put("faces", faces); h.put("face_index", fi)
    for p in range(P):
        h.put("rgb%d" % p, passes[p]); h.put("grad%d" % p, grads[p])
    # the tables of P device pointers, built from the held tensors
    h.put("rgb_table", np.array([h.addr("rgb%d" % p) for p in range(P)], np.int64))
    h.put("grad_table", np.array([h.addr("grad%d" % p) for p in range(P)], np.int64))
    h.put("mask_ws", np.full(8 * B * is_ * is_, 0xA5, np.uint8))          # not clear: the kernel must not rely on that
    ru.guarded(h, "grad_faces", (B, F, 3, 3))
    h.launchable()
    L.check(L.lib().sln_raster_backward_rgb_multi(h.p("faces"), h.p("face_index"), h.p("rgb_table"), h.p("grad_table"), P, B, F, is_, rc.EPS,
                                                  h.p("mask_ws"), h.p("grad_faces"), L.current_stream_ptr()), "backward_rgb_multi")
    _sync("sln_raster_backward_rgb_multi")
    return ru.read_guarded(h, "grad_faces", (B, F, 3, 3))


def _run_depth(faces, fi, w, d, gd, prefill=None):
    L = _lib()
    B, F = faces.shape[:2]
    is_ = fi.shape[1]
    assert faces.shape == (B, F, 3, 3) and fi.shape == d.shape == gd.shape == (B, is_, is_) and w.shape == (B, is_, is_, 3)
    ru.check_index_map("face_index", fi, F)
    h = ru.Operands()
    for k, a in (("faces", faces), ("face_index", fi), ("weight", w), ("depth", d), ("grad_depth", gd)):
        h.put(k, a)
    ru.guarded(h, "grad_faces", (B, F, 3, 3), prefill)
    h.launchable()
    L.check(L.lib().sln_raster_backward_depth(h.p("faces"), h.p("face_index"), h.p("weight"), h.p("depth"), h.p("grad_depth"), B, F, is_,
                                              h.p("grad_faces"), L.current_stream_ptr()), "backward_depth")
    _sync("sln_raster_backward_depth")
    return ru.read_guarded(h, "grad_faces", (B, F, 3, 3))


def _run_scene(faces, cls, gfin):
    """final [B,70,is,is] and grad_faces [B,F,3,3] (overwritten by the call: prefilled with SENT)"""
    L = _lib()
    B, F = faces.shape[:2]
    is_, NC = gfin.shape[-1], len(rc.SCENE_CHAN)
    assert faces.shape == (B, F, 3, 3) and cls.shape == (B, F) and gfin.shape == (B, 70, is_, is_) and len(rc.SCENE_DCH) == NC
    ru.check_index_list("face_class", cls, NC, lo=-1)
    ru.check_index_list("class_channel", rc.SCENE_CHAN, 40)
    ru.check_index_list("class_depth_channel", rc.SCENE_DCH, 29, lo=-1)
    h = ru.Operands()
    for k, a in (("faces", faces), ("face_class", cls), ("chan", rc.SCENE_CHAN), ("dch", rc.SCENE_DCH), ("grad_final", gfin)):
        h.put(k, a)
    h.put("workspace", torch.zeros(int(L.lib().sln_scene_workspace_bytes(B, F, is_)), dtype=torch.uint8, device="cuda"))
    ru.guarded(h, "final", (B, 70, is_, is_), fill=SENT)
    ru.guarded(h, "grad_faces", (B, F, 3, 3), fill=SENT)
    h.launchable()
    st = L.current_stream_ptr()
    L.check(L.lib().sln_scene_forward(h.p("faces"), h.p("face_class"), B, F, is_, NC, h.p("chan"), h.p("dch"), 0.1, 0.001, 100.0, 1e-3,
                                      h.p("workspace"), h.p("final"), st), "scene_forward")
    _sync("sln_scene_forward")
    L.check(L.lib().sln_scene_backward(h.p("faces"), h.p("face_class"), B, F, is_, NC, h.p("chan"), h.p("dch"), rc.EPS, h.p("workspace"),
                                       h.p("grad_final"), h.p("grad_faces"), st), "scene_backward")
    _sync("sln_scene_backward")
    return ru.read_guarded(h, "final", (B, 70, is_, is_)), ru.read_guarded(h, "grad_faces", (B, F, 3, 3))


def _split_pm(B, F, det=False):
    return "pixel_map_scan_split %d" % (1 if det else rc.pixel_map_scan_split(B, F))


def _split_depth(B, F, det=False):
    return "depth_bwd_split %d" % (1 if det else rc.depth_bwd_split(B, F))


# ---------------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DENSE) + ["room"])
def test_dense(name):
    (faces, fi, rgb, grad), (g64, S, n) = _dense(name)
    got = _run_dense(faces, fi, rgb, grad)
    _report("dense", name, ru.compare("dense " + name, got, g64, S, n, _split_pm(*faces.shape[:2])))


@pytest.mark.parametrize("name", list(MULTI))
def test_multi(name):
    (faces, fi, passes, grads), (g64, S, n) = _multi(name)
    got = _run_multi(faces, fi, passes, grads)
    _report("multi", name, ru.compare("multi " + name, got, g64, S, n, _split_pm(*faces.shape[:2])))


@pytest.mark.parametrize("name", list(DEPTH))
def test_depth(name):
    (faces, fi, w, d, gd), (g64, S, n) = _depth(name)
    got = _run_depth(faces, fi, w, d, gd)
    _report("depth", name, ru.compare("depth " + name, got, g64, S, n, _split_depth(*faces.shape[:2])))


def _check_scene(name, det=False):
    (faces, cls, gfin), (final, g64, S, n) = _scene(name)
    got_final, got = _run_scene(faces, cls, gfin)
    # a forward difference is reported as one: per value 1e-4, what test_refine_golden_gpu.py allows the scene image (no pixel may flip here)
    d = np.abs(got_final.astype(np.float64) - final)
    assert np.isfinite(got_final).all() and d.max() <= 1e-4, "scene %s: the FORWARD image differs from the reference's by %.3g at %s" % (
        name, d.max(), np.unravel_index(int(np.argmax(d)), d.shape))
    B, F = faces.shape[:2]
    res = ru.compare("scene " + name, got, g64, S, n, _split_pm(B, F, det) + ", " + _split_depth(B, F, det))
    _report("scene" + (" det" if det else ""), name, res)
    return got


@pytest.mark.parametrize("name", list(SCENE))
def test_scene(name):
    _check_scene(name)


@pytest.mark.parametrize("group,name", DET, ids=["%s-%s" % d for d in DET])
def test_deterministic_mode(group, name):
    """split 1 everywhere and another association: the same bound, and the same bits on a second run"""
    with _deterministic():
        runs = []
        for _ in range(2):
            if group == "dense":
                inp, (g64, S, n) = _dense(name)
                got = _run_dense(*inp)
                res = ru.compare("dense det " + name, got, g64, S, n, _split_pm(*inp[0].shape[:2], det=True))
            elif group == "multi":
                inp, (g64, S, n) = _multi(name)
                got = _run_multi(*inp)
                res = ru.compare("multi det " + name, got, g64, S, n, _split_pm(*inp[0].shape[:2], det=True))
            elif group == "depth":
                inp, (g64, S, n) = _depth(name)
                got = _run_depth(*inp)
                res = ru.compare("depth det " + name, got, g64, S, n, _split_depth(*inp[0].shape[:2], det=True))
            else:
                got, res = _check_scene(name, det=True), None
            runs.append(got)
        if res is not None:
            _report(group + " det", name, res)
    assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32)), "%s %s: two deterministic runs differ in %d values" % (
        group, name, int((runs[0].view(np.int32) != runs[1].view(np.int32)).sum()))


@pytest.mark.parametrize("group,name", [("dense", "B2-is130"), ("depth", "B9-is65")])
def test_adds_onto_the_callers_gradient(group, name):
    """grad_faces += : a prefill in multiples of 1/8 stays where no term exists and is part of the sum elsewhere; the allowance is the
    bound plus one ulp of |prefill| + |g64| (the last addition onto the prefill)"""
    inp, (g64, S, n) = _dense(name) if group == "dense" else _depth(name)
    pre = rc.eighths(np.random.default_rng(11), g64.shape)
    got = (_run_dense if group == "dense" else _run_depth)(*inp, prefill=pre)
    B, F = inp[0].shape[:2]
    _report(group + " +=", name, ru.compare(group + " += " + name, got, g64, S, n, (_split_pm if group == "dense" else _split_depth)(B, F),
                                            prefill=pre))


# ---------------------------------------------------------------------------------------------------------------------------------
# projection backward, both kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _proj(name):
    c = {c.name: c for c in ru.PROJ}[name]
    inp = ru.proj_inputs(c)
    return c, inp, ru.project_bwd_ref(*inp[:5], 512.0, 1e-9, inp[5])


def _run_project_bwd(c, verts, faces, K, R, t, gout, exempt):
    L = _lib()
    assert verts.shape == (c.B, c.V, 3) and faces.shape == (c.B, c.F, 3) and gout.shape == (c.B, c.F, 3, 3)
    assert K.shape == R.shape == (c.B, 3, 3) and t.shape == (c.B, 1, 3)
    ru.check_index_list("faces", faces, c.V, exempt=exempt)              # only the planted -1 / V corners, which both kernels skip
    h = ru.Operands()
    for k, a in (("vertices", verts), ("faces", faces), ("K", K), ("R", R), ("t", t), ("grad_faces_xyz", gout)):
        h.put(k, a)
    ru.guarded(h, "grad_vertices", (c.B, c.V, 3), fill=SENT)             # overwritten: the deterministic kernel stores, the other adds onto a zero fill
    h.launchable()
    L.check(L.lib().sln_project_faces_backward(h.p("vertices"), h.p("faces"), h.p("K"), h.p("R"), h.p("t"), c.B, c.V, c.F, 512.0, 1e-9,
                                               h.p("grad_faces_xyz"), h.p("grad_vertices"), L.current_stream_ptr()), "project_faces_backward")
    _sync("sln_project_faces_backward")
    return ru.read_guarded(h, "grad_vertices", (c.B, c.V, 3))


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("name", [c.name for c in ru.PROJ])
def test_project_faces_backward(name, det):
    c, inp, (g64, S, n) = _proj(name)
    if det:
        with _deterministic():
            got = _run_project_bwd(c, *inp)
            again = _run_project_bwd(c, *inp)
        assert np.array_equal(got.view(np.int32), again.view(np.int32))
    else:
        got = _run_project_bwd(c, *inp)
    res = ru.compare("projection " + name, got, g64, S, n, "deterministic" if det else "atomic", bound=ru.proj_bound,
                     what=("image", "vertex"))
    _report("projection " + ("det" if det else "atomic"), name, res)
