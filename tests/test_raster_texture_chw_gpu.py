"""sln_raster_texture_sample_chw against the float64 restatement of raster_bwd_gpu_util.py (run with -m gpu).

The index map is an operand of the kernel, which forms the face and texture addresses from it: the helper checks every map on the
host to lie in [-1, F) and holds every operand until after the synchronisation (LAB_NOTES section 25 on why)."""
import numpy as np
import pytest

import raster_bwd_cases as rc
import raster_bwd_gpu_util as ru
from gpu_util import _lib, _sync

pytestmark = pytest.mark.gpu

EPS = 1e-3


def _sample(faces, tex, fi, w, d, ts, scale):
    L = _lib()
    B, F = faces.shape[:2]
    F_tex, is_ = tex.shape[1], fi.shape[1]
    ru.check_index_map("face_index", fi, F)
    assert faces.shape == (B, F, 3, 3) and fi.shape == (B, is_, is_) and tex.shape == (B, F_tex, ts, ts, ts, 3) and w.shape == (B, is_, is_, 3) and d.shape == (B, is_, is_)
    h = ru.Operands()
    for k, a in (("faces", faces), ("textures", tex), ("face_index", fi), ("weight", w), ("depth", d)):
        h.put(k, a)
    ru.guarded(h, "rgb_chw", (B, 3, is_, is_), fill=ru.SENT)            # every output value is written, background included
    h.launchable()
    L.check(L.lib().sln_raster_texture_sample_chw(h.p("faces"), h.p("textures"), h.p("face_index"), h.p("weight"), h.p("depth"), B, F, F_tex,
                                                  is_, ts, EPS, scale, h.p("rgb_chw"), L.current_stream_ptr()), "texture_sample_chw")
    _sync("sln_raster_texture_sample_chw")
    return ru.read_guarded(h, "rgb_chw", (B, 3, is_, is_))


@pytest.mark.parametrize("index_map", ["forward", "random"])
@pytest.mark.parametrize("half,scale", [(False, 1.0), (True, 0.5), (True, 1.0), (False, 0.5)])
@pytest.mark.parametrize("is_,B,ts", [(8, 1, 2), (8, 3, 4), (65, 1, 4), (65, 3, 2)])
def test_texture_sample_chw(is_, B, ts, half, scale, index_map):
    """every output value within TEX_C(ts) 2^-24 sum |weight * texel| scale of the restatement, background exactly 0"""
    faces, tex, fi, w, d = ru.tex_inputs(is_, B, ts, half, index_map)
    got = _sample(faces, tex, fi, w, d, ts, scale)
    ref, A = ru.texture_chw_ref(faces, tex, fi, w, d, ts, EPS, scale)
    assert np.isfinite(got).all()
    bg = np.broadcast_to(np.flip(fi, 1)[:, None] < 0, ref.shape)
    assert bg.any() and (~bg).any()
    assert np.all(got[bg] == 0), "background pixels are not exactly 0"
    err, tol = np.abs(got - ref), ru.TEX_C(ts) * rc.U * A
    ratio = np.where(bg, 0.0, err / np.maximum(tol, 1e-300))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("texture is=%d B=%d ts=%d half=%d scale=%g %s: worst err / allowed %.3f at (image, channel, row, column) %s" % (
        is_, B, ts, half, scale, index_map, ratio[i], tuple(int(v) for v in i)))
    assert np.all(err <= tol), "worst err / allowed %.2f at (image, channel, row, column) %s: got %.9g want %.9g" % (
        ratio[i], i, got[i], ref[i])
