"""The split wgrad body (csrc/gemm_bodies.h::gemm_tn_split_body: operands as three bf16 parts, six products per k-step on the 16-bit
matrix pipe) at operand level, through the three launches that carry it: `sln_debug_gemm_tn` single and per-pass, and
`sln_debug_gemm_tn_mixed`.  Word 1 (sln_set_tn_split) against the fp64 reference of tests/gemm_ref.py at the family's own bounds (1e-5
relative and absolute on dW and db, tests/test_gemm_family_gpu.py); word 0's error on the same case is printed beside it.  The budget
is tests/test_tn_split_host.py's: the split drops 2^-24 of every product, fp32 accumulation rounds by as much.

Rows 1, 15, 16, 17, 31, 33 (around the 16-row k-step of a wave and the 32-row tile), 705 and 1 409 (one row past one / two 704-row
chunks); widths 6 (rows of 8), 24, 64, 96, 130 as Nout and as Kin; plain and gathered X with both index arrays; one- and two-source G;
with and without db; a gathered problem among plain ones.
Range: bf16 parts have fp32's exponents, so scaling an operand by 2^-40 or 2^+40 scales dW and db by exactly that - bit for bit with
one chunk per problem (one add per element).  A NaN in G reaches the output rows of its column and no other.  A problem with
sgd_step keeps the fp32 body: word 1 gives word 0's bits."""
import numpy as np
import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
import test_tn_mixed_gpu as MX
from gpu_util import Dev, _lib, _sync, _assert_close

pytestmark = pytest.mark.gpu

ROWS = (1, 15, 16, 17, 31, 33, 705, 1409)
WIDTHS = (6, 24, 64, 96, 130)


@pytest.fixture
def lib():
    h = _lib().lib()
    word, det = h.sln_get_tn_split(), h.sln_get_deterministic()
    yield h
    assert h.sln_set_tn_split(word) == 0
    h.sln_set_deterministic(det)


def _launch(L, probs, route, dev, steps=None):
    n = len(probs)
    descs = (L.SlnDbgGemmTN * n)()
    outs = []
    for i, p in enumerate(probs):
        dW = p.dW0.cuda().clone()
        db = None if p.db0 is None else p.db0.cuda().clone()
        step = None if p.sgd_step is None else torch.tensor([p.sgd_step], dtype=torch.float32, device="cuda")
        descs[i] = GC.tn_desc(L, p, dev, dW, db, step)
        outs.append((dW, db, step))
    if route == "mixed":
        rc = L.lib().sln_debug_gemm_tn_mixed(descs, n, L.current_stream_ptr())
    else:
        rc = L.lib().sln_debug_gemm_tn(descs, n, 1 if route == "perpass" else 0, L.current_stream_ptr())
    _sync("wgrad launch (%s), %d problems, split word %d" % (route, n, L.lib().sln_get_tn_split()))
    assert rc == 0, "%s launch returned %d" % (route, rc)
    return [(dW.cpu(), None if db is None else db.cpu()) for dW, db, _ in outs]


def _both_words(lib, probs, route):
    """-> {word: outputs}; one upload of the operands for both."""
    L, dev, out = _lib(), Dev(), {}
    for word in (0, 1):
        assert lib.sln_set_tn_split(word) == 0
        out[word] = _launch(L, probs, route, dev)
    return out


def _err(p, dW, db):
    rW, rb = R.tn(p)
    eW = float((dW[:, :p.Kin].double() - rW).abs().max())
    eb = None if rb is None else float((db.double() - rb).abs().max())
    return eW, eb


def _check(p, out, i, tag):
    """Word 1 at the family's bounds; word 0's error beside it."""
    rW, rb = R.tn(p)
    dW1, db1 = out[1][i]
    e0W, e0b = _err(p, *out[0][i])
    assert torch.equal(dW1[:, p.Kin:], p.dW0[:, p.Kin:]), "%s: wrote behind column Kin" % tag
    e, tol = _assert_close(dW1[:, :p.Kin], rW, 1e-5, 1e-5, tag + " dW", MX._form(p))
    line = "%s: dW err split %.3e fp32 %.3e bound %.3e" % (tag, e, e0W, tol)
    if rb is not None:
        eb, tb = _assert_close(db1, rb, 1e-5, 1e-5, tag + " db", MX._form(p))
        line += " | db err split %.3e fp32 %.3e bound %.3e" % (eb, e0b, tb)
    print(line)


def _lists():
    # every row count: plain and gathered ('concat': both index arrays), one- and two-source G, with and without db (every third without)
    rows = []
    for i, Rr in enumerate(ROWS):
        # (one row: plain G only - a two-source G is a BatchNorm backward, and over ONE row its statistics have no spread: the fp32
        #  coefficients alone are 1e-4 off the fp64 ones, in either body)
        rows.append((Rr, 96, 96, "bwd" if i % 2 else "plain", "concat"))
        rows.append((Rr, 64, 24, "plain" if i % 2 or Rr == 1 else "bwd", "relu" if i % 2 else "ident"))
    # every width as Nout and as Kin, in both bodies and both G forms
    widths = []
    for i, w in enumerate(WIDTHS):
        widths.append((300, w, WIDTHS[(i + 2) % 5], "plain" if i % 2 else "bwd", "relu"))
        widths.append((300, WIDTHS[(i + 1) % 5], w, "bwd" if i % 2 else "plain", "gather"))
    widths.append((70, 130, 130, "bwd", "ident"))
    widths.append((33, 6, 6, "plain", "gather"))
    return {"rows": rows, "widths": widths,
            "one-gathered": [(300, 24, 100, "plain", "relu"), (1000, 100, 96, "bwd", "concat"), (13, 8, 36, "plain", "ident")],
            "one-plain": [(300, 24, 96, "plain", "concat"), (70, 100, 100, "bwd", "relu"), (1409, 96, 24, "plain", "gather")]}


LISTS = _lists()


def _problems(key):
    return [MX._problem("split-%s-%d" % (key, i), Rr, Nout, Kin, gf, xf, with_db=(i % 3 != 2)) for i, (Rr, Nout, Kin, gf, xf) in enumerate(LISTS[key])]


@pytest.mark.parametrize("route", ["perpass", "mixed"])
@pytest.mark.parametrize("key", sorted(LISTS))
def test_table_launches(lib, key, route):
    probs = _problems(key)
    if route == "perpass":                   # the per-pass hook takes whole groups of four columns only: 6 and 130 run in the mixed launch
        probs = [p for p in probs if p.Nout % 4 == 0 and p.Kin % 4 == 0]
    out = _both_words(lib, probs, route)
    for i, p in enumerate(probs):
        _check(p, out, i, "%s/%s[%d] (%d, %d, %d)" % (route, key, i, p.R, p.Nout, p.Kin))


# the single launch alone (a sixth entry: rows_per_block).  'surplus': three 32-row tiles per chunk - the K loop runs whole pairs of
# tiles, so the rows of a fourth are staged as zeros - in three chunks, the last of 8 rows; two ragged output tiles each way
SINGLE = dict(LISTS, surplus=[(200, 100, 100, "bwd", "concat", 96)])


@pytest.mark.parametrize("key", ["rows", "widths", "surplus"])
def test_single_launch(lib, key):
    """Widths of a single launch must be whole groups of four (the hook's rule for it): the others go through the tables above."""
    for i, (Rr, Nout, Kin, gf, xf, *rpb) in enumerate(SINGLE[key]):
        if Nout % 4 or Kin % 4:
            continue
        p = MX._problem("split-single-%s-%d" % (key, i), Rr, Nout, Kin, gf, xf, with_db=(i % 3 != 2))
        if rpb:
            p = p.replace(rows_per_block=rpb[0])
        out = _both_words(lib, [p], "single")
        _check(p, out, 0, "single/%s[%d] %s" % (key, i, SINGLE[key][i]))
        if Rr >= 300:            # (a sum over a few rows can round alike in both bodies)
            assert not torch.equal(out[1][0][0], out[0][0][0]), "word 1 gave word 0's bits: the single launch did not take the split body"


def _scaled(p, which, s):
    """The problem with the stored sources of operand `which` ('G' / 'X') multiplied by s (identity segments: the operand itself)."""
    op = getattr(p, which)
    segs = tuple(sg.replace(x1=sg.x1 * s) for sg in op.segs)
    return p.replace(**{which: op.replace(segs=segs)})


@pytest.mark.parametrize("route", ["single", "perpass", "mixed"])
@pytest.mark.parametrize("xf", ["ident", "gather"])
def test_a_power_of_two_scale_goes_through_bit_for_bit(lib, route, xf):
    """One chunk per problem (R = 705 <= the planner's chunk; rows_per_block set for the single launch): every dW / db element gets
    one add onto zeros, so the result is the workgroup's own sum.  Scaling G (or X) by 2^-40 / 2^+40 scales every part of the split,
    every product and every partial sum by exactly that: the outputs must be the unscaled ones times the factor, bit for bit.  An fp16
    split could not do this (2^-40 is below its smallest subnormal)."""
    assert lib.sln_set_tn_split(1) == 0
    L = _lib()
    g = GC._seed("split-scale", route, xf)
    Rr, Nout, Kin = 705, 96, 64
    p = MX._problem("split-scale-%s" % xf, Rr, Nout, Kin, "plain", xf)
    if xf == "gather":                                   # an identity view of the gathered source: the scale must commute with it
        p = p.replace(X=p.X.replace(segs=(MX._seg(g, p.X.segs[0].x1.shape[0], Kin, "ident", 0, 2),)))
    p = p.replace(dW0=torch.zeros_like(p.dW0), db0=torch.zeros_like(p.db0), rows_per_block=704 + 32 if route == "single" else 0)
    ((dW, db),) = _launch(L, [p], route, Dev())
    assert float(dW.abs().max()) > 0 and float(db.abs().max()) > 0
    for which in ("G", "X"):
        for e in (-40, 40):
            s = 2.0 ** e
            ((dWs, dbs),) = _launch(L, [_scaled(p, which, s)], route, Dev())
            assert torch.equal(dWs, dW * s), "%s x 2^%d: dW is not the unscaled dW x 2^%d" % (which, e, e)
            assert torch.equal(dbs, db * s if which == "G" else db), "%s x 2^%d: db" % (which, e)


@pytest.mark.parametrize("route", ["single", "perpass", "mixed"])
def test_a_nan_in_g_reaches_its_output_rows_and_no_other(lib, route):
    """NaNs in three columns of one row of G.  The operand transform both bodies share ends in v_max_f32 against the column's floor
    (csrc/gemm_bodies.h: sln_vmax; -3e38 for an identity column), which returns the floor for a NaN: what reaches the products is
    -3e38, in the fp32 body as here.  So the poisoned value is told by its size, not by isnan: every element of the three output rows
    (and their db) is non-finite or beyond 1e30, and every other row is, bit for bit, the row of the run without the NaNs (one chunk:
    one add per element) - a part of the split that leaked into a neighbouring column, or a transposed read that took another
    lane's rows, would show there."""
    assert lib.sln_set_tn_split(1) == 0
    L = _lib()
    Rr, Nout, Kin = 705, 96, 64
    p = MX._problem("split-nan", Rr, Nout, Kin, "plain", "ident").replace(rows_per_block=736 if route == "single" else 0)
    ((cW, cb),) = _launch(L, [p], route, Dev())
    x1 = p.G.segs[0].x1.clone()
    c1 = p.G.segs[0].c1
    hit = (3, 40, 95)                                   # G columns = dW rows; all in row 517 of G (the second k-step of a tile)
    for n in hit:
        x1[517, c1 + n] = float("nan")
    q = p.replace(G=p.G.replace(segs=(p.G.segs[0].replace(x1=x1),)))
    descs = (L.SlnDbgGemmTN * 1)()
    dev = Dev()
    dW, db = q.dW0.cuda().clone(), q.db0.cuda().clone()
    descs[0] = GC.tn_desc(L, p, dev, dW, db, None)      # (described from the clean problem: the reference-side checks refuse a NaN)
    descs[0].G = GC._operand_desc(L, q.G, dev)
    if route == "mixed":
        rc = L.lib().sln_debug_gemm_tn_mixed(descs, 1, L.current_stream_ptr())
    else:
        rc = L.lib().sln_debug_gemm_tn(descs, 1, 1 if route == "perpass" else 0, L.current_stream_ptr())
    _sync("wgrad launch with NaNs in G (%s)" % route)
    assert rc == 0
    dW, db = dW.cpu(), db.cpu()
    want = torch.zeros(Nout, dtype=torch.bool)
    want[list(hit)] = True
    big = ~torch.isfinite(dW[:, :Kin]) | (dW[:, :Kin].abs() > 1e30)
    assert bool(big[want].all()), "an element of a poisoned output row is neither non-finite nor beyond 1e30"
    assert torch.equal(dW[~want], cW[~want]), "rows %s changed" % sorted(set((dW != cW).nonzero()[:, 0].tolist()) - set(hit))
    bigb = ~torch.isfinite(db) | (db.abs() > 1e30)
    assert bool(bigb[want].all()) and torch.equal(db[~want], cb[~want])


@pytest.mark.parametrize("route", ["single", "perpass", "mixed"])
def test_an_sgd_problem_keeps_the_fp32_body(lib, route):
    """sgd_step set: word 1 must give word 0's bits (one chunk: one add per element, nothing depends on arrival order)."""
    L = _lib()
    p = MX._problem("split-sgd", 300, 24, 96, "bwd", "relu").replace(sgd_step=0.0625 + 1.0 / 3.0)
    q = MX._problem("split-sgd-other", 300, 24, 96, "plain", "relu")      # a problem that does take the split, in the same table
    probs = [p] if route == "single" else [p, q]
    out = _both_words(lib, probs, route)
    assert torch.equal(out[1][0][0], out[0][0][0]) and torch.equal(out[1][0][1], out[0][0][1]), "the sgd problem changed with the word"
    rW, rb = R.tn(p)
    _assert_close(out[1][0][0][:, :p.Kin], rW, 1e-5, 1e-5, "sgd dW", MX._form(p))
    if route != "single":
        assert not torch.equal(out[1][1][0], out[0][1][0]), "the plain problem beside it did not take the split body"
        _check(q, out, 1, "%s/beside-sgd" % route)


def test_deterministic_mode_keeps_the_fp32_body(lib):
    L = _lib()
    probs = _problems("one-gathered")
    lib.sln_set_deterministic(1)
    out = _both_words(lib, probs, "mixed")
    for i in range(len(probs)):
        assert torch.equal(out[1][i][0], out[0][i][0]), "problem %d: dW differs between the words in deterministic mode" % i
