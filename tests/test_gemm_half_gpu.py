"""The fp16-MFMA NT kernel (csrc/gemm_half.hip; precision modes "f16" = 1 product, "f16x3" = 3 products) at operand level through
sln_debug_gemm_nt_half, against the fp64 reference of tests/gemm_ref.py.  Every element is compared; SENT sentinels sit left and
right of the column window.

Bounds.  e32 is the error of the existing fp32 route on the same problem (sln_debug_gemm_nt), yard that of gemm_ref in float32: two
yardsticks from outside the new code.  As in test_spade_f16_gpu.py, bound = 2 max(e32, yard) + 1e-7 max(1, max |ref|).
  3 products: against fp64 of the SPLIT operands (hi / lo of a float32 CPU evaluation of op(A) and of W, three products in fp64) the
     error is <= bound; against fp64 of the unrounded operands <= bound + e_split, e_split the distance of the two references.
  1 product, identity operands: against fp64 of the fp16-rounded operands <= bound.
  1 product, affine operands: an ulp in the fp32 transform can move an fp16 rounding, so the comparison is element by element with
     the unrounded reference: <= 2^-10 (|A| |W|^T) + bound (two factors rounded to 11 bits: 2 x 2^-11 + 2^-22 per product)."""
import ctypes as C

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
from gpu_util import SENT, Dev, _lib, _sync

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2

# (M, N, K, segment lens, operand mode, variant of gemm_cases): what each covers is in the id
CASES = [
    ("one-row", 1, 32, 32, None, "ident", 0),
    ("one-step-ragged-M", 33, 32, 16, None, "ident", 1),
    ("boundary-in-chunk-evalbn-gathers", 70, 96, 144, (64, 64, 16), "affine", 5),
    ("net1.0", 200, 256, 384, (128, 128, 128), "affine", 0),
    ("net1.1-relu", 133, 640, 256, None, "affine", 2),
    ("net2.1", 300, 64, 256, None, "ident", 0),
]
BY_NAME = {c[0]: c for c in CASES}
_problems, _refs = {}, {}


def _problem(name):
    if name not in _problems:
        _, M, N, K, lens, mode, v = BY_NAME[name]
        p = GC.nt_problem("half-" + name, M, N, K, lens, mode, R.EPI_PLAIN, -1, v).replace(addend=None, ycol0=4, ldy=N + 12)
        if name.startswith("boundary"):           # eval-mode BatchNorm on all three segments (gemm_cases gives the gathered ones batch statistics)
            g = torch.Generator().manual_seed(77)
            p = p.replace(A=p.A.replace(segs=tuple(s.replace(bn=GC.bn_eval(g, s.len)) for s in p.A.segs)))
        _problems[name] = p
    return _problems[name]


def _f16(t):
    return t.clamp(-65504.0, 65504.0).half().double()


def _launch(L, p, dev, terms):
    """terms 0: the existing fp32 route."""
    Y = torch.full((p.M, p.ldy), SENT, device="cuda")
    d = GC.nt_desc(L, p, dev, Y=Y)
    if terms:
        rc = L.lib().sln_debug_gemm_nt_half(C.byref(d), terms, L.current_stream_ptr())
    else:
        rc = L.lib().sln_debug_gemm_nt(C.byref(d), 1, None, L.current_stream_ptr())
    _sync("%s, M %d N %d K %d" % ("sln_debug_gemm_nt_half terms %d" % terms if terms else "sln_debug_gemm_nt", p.M, p.N, p.K))
    assert rc == 0, rc
    Y = Y.cpu()
    lo, hi = p.ycol0, p.ycol0 + p.N
    assert bool((Y[:, :lo] == SENT).all()) and bool((Y[:, hi:] == SENT).all()), "wrote outside its column window"
    return Y[:, lo:hi]


def _references(L, p, dev, key):
    """Computed once per problem, never modified: the references and the bound."""
    if key not in _refs:
        ref = R.nt(p)["y"]
        yard = float((R.nt(p, torch.float32)["y"].double() - ref).abs().max())
        e32 = float((_launch(L, p, dev, 0).double() - ref).abs().max())
        bound = 2.0 * max(e32, yard) + 1e-7 * max(1.0, float(ref.abs().max()))
        A32 = R.operand(p.A, p.M, torch.float32).double()
        W32 = p.W[:p.N, :p.K].double()
        Ah, Wh = _f16(A32), _f16(W32)
        Al, Wl = _f16(A32 - Ah), _f16(W32 - Wh)
        b = 0.0 if p.bias is None else p.bias[:p.N].double()
        split = Ah @ Wl.t() + Al @ Wh.t() + Ah @ Wh.t() + b
        rounded = Ah @ Wh.t() + b
        absprod = R.operand(p.A, p.M).abs() @ W32.abs().t()
        _refs[key] = dict(ref=ref, yard=yard, e32=e32, bound=bound, split=split, rounded=rounded, absprod=absprod,
                          e_split=float((split - ref).abs().max()))
    return _refs[key]


def _first_bad(err, tol):
    bad = (err > tol).nonzero()
    return tuple(int(v) for v in bad[0]) if bad.numel() else None


def _check(p, r, Y3, Y1, ident, tag):
    y3, y1 = Y3.double(), Y1.double()
    e3s, e3 = (y3 - r["split"]).abs(), (y3 - r["ref"]).abs()
    print("%s: e32 %.3e yard %.3e bound %.3e e_split %.3e | f16x3 vs split %.3e vs fp64 %.3e | f16 vs rounded %.3e vs fp64 %.3e" % (
        tag, r["e32"], r["yard"], r["bound"], r["e_split"], float(e3s.max()), float(e3.max()), float((y1 - r["rounded"]).abs().max()),
        float((y1 - r["ref"]).abs().max())))
    assert bool(torch.isfinite(y3).all()) and bool(torch.isfinite(y1).all()), tag
    assert float(e3s.max()) <= r["bound"], "%s f16x3 vs split operands: %.3e > %.3e at %s" % (tag, float(e3s.max()), r["bound"], _first_bad(e3s, r["bound"]))
    assert float(e3.max()) <= r["bound"] + r["e_split"], "%s f16x3 vs fp64: %.3e > %.3e" % (tag, float(e3.max()), r["bound"] + r["e_split"])
    if ident:
        e1 = (y1 - r["rounded"]).abs()
        assert float(e1.max()) <= r["bound"], "%s f16 vs rounded operands: %.3e > %.3e at %s" % (tag, float(e1.max()), r["bound"], _first_bad(e1, r["bound"]))
    else:
        e1, tol = (y1 - r["ref"]).abs(), 2.0 ** -10 * r["absprod"] + r["bound"]
        assert bool((e1 <= tol).all()), "%s f16 vs fp64, element by element: first failing %s, worst ratio %.3f" % (
            tag, _first_bad(e1, tol), float((e1 / tol).max()))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_half_kernel_against_fp64(case, bias):
    L = _lib()
    name, mode = case[0], case[5]
    p = _problem(name) if bias else _problem(name).replace(bias=None)
    dev = Dev()
    r = _references(L, p, dev, (name, bias))
    Y3, Y1 = _launch(L, p, dev, 3), _launch(L, p, dev, 1)
    _check(p, r, Y3, Y1, mode == "ident", "%s[%s]" % (name, "bias" if bias else "nobias"))
    if name == "net2.1":                          # the one-product mode really rounds
        far = float((Y1.double() - r["ref"]).abs().max())
        assert far > 10.0 * r["bound"], (far, r["bound"])


def test_rows_do_not_depend_on_m_and_launches_repeat():
    L = _lib()
    p = _problem("net2.1")
    dev = Dev()
    for terms in (3, 1):
        full = _launch(L, p, dev, terms)
        assert torch.equal(full, _launch(L, p, dev, terms)), "two launches of one problem differ (terms %d)" % terms
        head = _launch(L, p.replace(M=5), dev, terms)
        assert torch.equal(head, full[:5]), "rows 0-4 of a 5-row launch differ from the 300-row launch (terms %d)" % terms


def _poke(p, row, col, value):
    """The same problem with one element of the (single, identity) operand replaced."""
    s = p.A.segs[0]
    x1 = s.x1.clone()
    x1[row, s.c1 + col] = value
    return p.replace(A=p.A.replace(segs=(s.replace(x1=x1),)))


def test_nan_reaches_its_row_only():
    L = _lib()
    p = _problem("net2.1")
    assert p.A.segs[0].which == 0 and p.A.segs[0].coef == R.COEF_IDENT
    q = _poke(p, 7, 13, float("nan"))
    dev = Dev()
    for terms in (3, 1):
        nan = torch.isnan(_launch(L, q, dev, terms))
        assert bool(nan[7].all()) and int(nan.sum()) == p.N, "terms %d: NaN in %d outputs, row 7 has %d" % (terms, int(nan.sum()), int(nan[7].sum()))


def test_operands_beyond_the_fp16_range_are_clamped():
    L = _lib()
    p = _problem("net2.1")
    big, clamped = _poke(p, 7, 13, 1.0e5), _poke(p, 7, 13, 65504.0)
    dev = Dev()
    r = _references(L, clamped, dev, "clamped")
    Y3, Y1 = _launch(L, big, dev, 3), _launch(L, big, dev, 1)
    _check(clamped, r, Y3, Y1, True, "1e5 in A against the clamped reference")
    assert float((r["ref"][7] - R.nt(big)["y"][7]).abs().max()) > 100.0 * r["bound"]          # the clamp is visible in this row


def test_refused_description_launches_nothing():
    L = _lib()
    p = GC.nt_problem("half-refused", 70, 24, 256, None, "affine", R.EPI_PLAIN, -1, 0).replace(addend=None, ycol0=4, ldy=36)
    dev = Dev()
    for q in (p, _problem("net2.1").replace(ycol0=3)):
        Y = torch.full((q.M, q.ldy), SENT, device="cuda")
        d = GC.nt_desc(L, q, dev, Y=Y)
        for terms in (3, 1):
            assert L.lib().sln_debug_gemm_nt_half(C.byref(d), terms, L.current_stream_ptr()) == UNSUPPORTED
        assert L.lib().sln_debug_gemm_nt_half(C.byref(d), 2, L.current_stream_ptr()) == -1      # not a mode
        torch.cuda.synchronize()
        assert bool((Y == SENT).all())
