"""The ONE wgrad launch of a full iteration (csrc/gemm_f32.hip::gemm_tn_mixed_kernel) at operand level: problems that gather
their input rows and problems that do not share a grid, every workgroup running the body its problem needs.  Through
`sln_debug_gemm_tn_mixed`, against the fp64 reference of tests/gemm_ref.py at the bounds of tests/test_gemm_family_gpu.py
(1e-5 relative and absolute on dW and db, scaled by the reference's max-abs where that exceeds 1).

Shapes: R = 1, 31, 33 (around one 32-row k-tile) and 705 (one row past the 704-row chunk of the 64-graph step: a last k-tile of
one row), 1409 and 2100 rows (two and three chunks); output and input widths of 6, 24, 96 and 130 (less than a group of four
columns past a multiple, one tile, more than one tile, two columns into a third tile); a gathered problem next to plain ones
whose index arrays are NULL; and a list of 70 problems / 4 200 workgroups, past the 64 problems and 4 096 items of the per-kind
launches."""
import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
from gpu_util import Dev, _lib, _sync, _assert_close

pytestmark = pytest.mark.gpu


def _seg(g, rows, length, mode, variant, which, c1=4):
    """GC._seg over the width rounded up to four columns, cut back to `length`: rows stay stored up to the group's end."""
    s = GC._seg(g, rows, (length + 3) & ~3, mode, variant, which, c1)
    return s.replace(len=length)


def _problem(key, Rr, Nout, Kin, gform, xform, with_db=True):
    """xform: 'ident' / 'relu' (plain rows, NO index arrays), 'gather' (one gathered segment), 'concat' ([obj[s] | pred | obj[o]]:
    two gathered thirds around a plain one; Kin must split into three multiples of four)."""
    g = GC._seed("mixed-" + key)
    G = R.Operand(segs=(_seg(g, Rr, Nout, "bwd" if gform == "bwd" else "ident", 0, 0),))
    n_obj = max(5, Rr // 2 + 3)
    if xform == "concat":
        a = (Kin // 3) & ~3
        lens = (a, Kin - 2 * a, a)
        assert all(v > 0 and v % 4 == 0 for v in lens[:2]), lens
        segs = (_seg(g, n_obj, lens[0], "affine", 0, 1, c1=0), _seg(g, Rr, lens[1], "affine", 2, 0), _seg(g, n_obj, lens[2], "ident", 0, 2, c1=0))
        X = R.Operand(segs=segs, idx_a=GC.gather_index(g, Rr, n_obj), idx_b=GC.gather_index(g, Rr, n_obj))
    elif xform == "gather":
        X = R.Operand(segs=(_seg(g, n_obj, Kin, "affine", 0, 2),), idx_b=GC.gather_index(g, Rr, n_obj))
    else:
        X = R.Operand(segs=(_seg(g, Rr, Kin, "affine" if xform == "relu" else "ident", 0, 0),))
        assert X.idx_a is None and X.idx_b is None
    return R.TN(G=G, X=X, R=Rr, Nout=Nout, Kin=Kin, dW0=GC._randn(g, Nout, Kin + 4), db0=GC._randn(g, Nout) if with_db else None)


# (R, Nout, Kin, G form, X form)
LISTS = {
    # every row count, gathered and plain side by side
    "rows": [(1, 24, 96, "plain", "ident"), (1, 24, 96, "plain", "concat"), (31, 96, 24, "bwd", "relu"), (31, 24, 96, "plain", "gather"),
             (33, 96, 96, "plain", "concat"), (33, 24, 24, "bwd", "ident"), (705, 96, 96, "bwd", "concat"), (705, 96, 24, "plain", "relu"),
             (1409, 24, 96, "plain", "ident"), (2100, 24, 36, "plain", "concat")],
    # every width as Nout and as Kin, in both bodies
    "widths": [(300, 6, 130, "plain", "ident"), (300, 130, 6, "plain", "relu"), (300, 6, 96, "plain", "gather"), (300, 130, 24, "bwd", "gather"),
               (300, 24, 130, "plain", "gather"), (300, 96, 6, "plain", "gather"), (300, 130, 130, "bwd", "ident"), (300, 24, 96, "plain", "concat"),
               (70, 96, 130, "plain", "relu"), (70, 6, 6, "plain", "ident")],
    # one gathered problem between plain ones without index arrays, and the reverse
    "one-gathered": [(300, 24, 100, "plain", "relu"), (1000, 100, 96, "bwd", "concat"), (13, 8, 36, "plain", "ident")],
    "one-plain": [(300, 24, 96, "plain", "concat"), (70, 100, 100, "bwd", "relu"), (1000, 96, 24, "plain", "gather")],
    "all-plain": [(300, 24, 100, "plain", "relu"), (705, 130, 24, "bwd", "ident")],
    "all-gathered": [(300, 24, 96, "plain", "concat"), (705, 130, 24, "bwd", "gather")],
}


def _launch(L, probs, dev):
    n = len(probs)
    descs = (L.SlnDbgGemmTN * n)()
    outs = []
    for i, p in enumerate(probs):
        dW = p.dW0.cuda().clone()
        db = None if p.db0 is None else p.db0.cuda().clone()
        descs[i] = GC.tn_desc(L, p, dev, dW, db, None)
        outs.append((dW, db))
    rc = L.lib().sln_debug_gemm_tn_mixed(descs, n, L.current_stream_ptr())
    _sync("sln_debug_gemm_tn_mixed, %d problems" % n)
    assert rc == 0, "sln_debug_gemm_tn_mixed returned %d" % rc
    return [(dW.cpu(), None if db is None else db.cpu()) for dW, db in outs]


def _form(p):
    return "mixed launch, G_X2=%d, gathered=%d" % (any(s.x2 is not None for s in p.G.segs), any(s.which for s in p.X.segs))


def _check(p, dW, db, tag):
    rW, rb = R.tn(p)
    assert torch.equal(dW[:, p.Kin:], p.dW0[:, p.Kin:]), "%s: wrote behind column Kin; %s" % (tag, _form(p))
    e, tol = _assert_close(dW[:, :p.Kin], rW, 1e-5, 1e-5, tag + " dW", _form(p))
    line = "%s: dW err %.3e bound %.3e" % (tag, e, tol)
    if rb is not None:
        eb, tb = _assert_close(db, rb, 1e-5, 1e-5, tag + " db", _form(p))
        line += " | db err %.3e bound %.3e" % (eb, tb)
    print(line)


@pytest.mark.parametrize("key", sorted(LISTS))
def test_mixed_list(key):
    L = _lib()
    probs = [_problem("%s-%d" % (key, i), Rr, Nout, Kin, gf, xf, with_db=(i % 3 != 2)) for i, (Rr, Nout, Kin, gf, xf) in enumerate(LISTS[key])]
    outs = _launch(L, probs, Dev())
    for i, p in enumerate(probs):
        _check(p, outs[i][0], outs[i][1], "%s[%d] %s" % (key, i, LISTS[key][i]))


def test_a_list_past_the_per_kind_limits():
    """70 problems of 60 output tiles each: more problems than one per-kind launch holds (64) and more workgroups (4 200) than its
    item table (4 096).  One chunk of 33 rows each, so the fp64 reference stays at a gigaflop; every third problem gathers."""
    L = _lib()
    probs = []
    for i in range(70):
        if i % 3 == 0:
            probs.append(_problem("long-%d" % i, 33, 640, 384, "plain", "concat", with_db=(i % 2 == 0)))
        else:
            probs.append(_problem("long-%d" % i, 33, 640, 384, "bwd" if i % 3 == 1 else "plain", "relu", with_db=(i % 2 == 0)))
    outs = _launch(L, probs, Dev())
    worst = 0.0
    for i, p in enumerate(probs):
        rW, rb = R.tn(p)
        e, tol = _assert_close(outs[i][0][:, :p.Kin], rW, 1e-5, 1e-5, "long[%d] dW" % i, _form(p))
        worst = max(worst, e / tol)
        if rb is not None:
            _assert_close(outs[i][1], rb, 1e-5, 1e-5, "long[%d] db" % i, _form(p))
    print("70 problems: worst dW error %.3f of its bound" % worst)


def test_the_hook_refuses_what_the_launch_cannot_take():
    L = _lib()
    p = _problem("refuse", 13, 8, 36, "plain", "ident")
    dev = Dev()
    dW = p.dW0.cuda().clone()
    d = GC.tn_desc(L, p, dev, dW, None, None)
    import ctypes as C
    assert L.lib().sln_debug_gemm_tn_mixed(C.byref(d), 0, L.current_stream_ptr()) == -1
    assert L.lib().sln_debug_gemm_tn_mixed(C.byref(d), 129, L.current_stream_ptr()) == -1
    d.G.seg[0].which = 1                                     # a gathered gradient operand
    assert L.lib().sln_debug_gemm_tn_mixed(C.byref(d), 1, L.current_stream_ptr()) == -1
    d.G.seg[0].which = 0
    d.X.seg[0].len, d.Kin = 34, 34                           # a ragged width whose rows end with it (ld = 44 >= 4 + 36 holds; shrink it)
    d.X.seg[0].ld1 = 36
    assert L.lib().sln_debug_gemm_tn_mixed(C.byref(d), 1, L.current_stream_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(dW.cpu(), p.dW0)
