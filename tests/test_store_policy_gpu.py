"""Write-through stores in the NT GEMM epilogues (sln_set_store_policy, csrc/sln_common.h) against plain stores, at operand level
through sln_debug_gemm_nt (run with -m gpu on an MI355X).

The policy picks another instantiation of the same body: only the cache policy of the 4-byte stores of Y moves.  So policy 1
against policy 0 is held to EQUALITY - every element of the output buffer, the sentinels left of, right of and below the written
slice included, and both rows of the fp64 column statistics (their partial sums are quantised so that they commute,
sln_common.h: sln_qd) - and the write-through result is held to the fp64 reference of tests/gemm_ref.py at the family's own
bounds (tests/test_gemm_family_gpu.py: rtol 2e-6 / atol 1e-6 on y, 1e-5 on the sums).

Shapes: M in {1, 31, 33, 64, 65, 100} x N in {6, 24, 96, 130, 160, 384, 640}, K in {32, 96, 256}, the three epilogues with and
without an addend, ldy > N with ycol0 in {0, 4, 6} and the buffer's base 4 bytes off a 16-byte boundary.  Each N is one test
that walks all six M; K, epilogue, addend and ycol0 cycle along so that every value meets every N and every M, and every second
case asks for the 64 x 64 body (the dispatcher's own choice at these sizes is the 32 x 32 split-K body).  The 16 x 16 body wants a
chip-filling M whatever is asked (nt16_pick), so two tall problems - the
row counts of tests/gemm_cases.py - run the J = 3 and J = 5 tiles.  The remaining instantiations that carry the store form - the
three-segment split-K body, the multi-segment forms of the 64 x 64 body, the 128 x 64 / 128 x 128 tiles, grouped launches with
single- and three-segment operands - run on rows of gemm_cases' own tables; the last test asserts that every body is covered."""
import ctypes as C

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
from gpu_util import SENT, Dev, _lib, _sync, _assert_close

pytestmark = pytest.mark.gpu

MS = (1, 31, 33, 64, 65, 100)
NS = (6, 24, 96, 130, 160, 384, 640)
KS = (32, 96, 256)
YCOL0 = (0, 4, 6)
MODE_OF_EPI = {R.EPI_PLAIN: "ident", R.EPI_STATS: "affine", R.EPI_MASK: "bwd"}


@pytest.fixture
def policy():
    h = _lib().lib()
    before = h.sln_get_store_policy()

    def set_(v):
        assert h.sln_set_store_policy(v) == 0 and h.sln_get_store_policy() == v
    yield set_
    assert h.sln_set_store_policy(before) == 0


def _buffers(p):
    """Y: rows of ldy floats starting 4 bytes behind a 256-byte aligned allocation, one sentinel row below the M written ones."""
    flat = torch.full(((p.M + 1) * p.ldy + 1,), SENT, device="cuda")
    assert flat.data_ptr() % 16 == 0
    Y = flat[1:].view(p.M + 1, p.ldy)
    S = torch.zeros(2, p.ocstride, dtype=torch.float64, device="cuda")
    S[:, p.N:] = SENT
    return flat, Y, S


def _launch(L, probs, dev):
    n = len(probs)
    descs = (L.SlnDbgGemmNT * n)()
    keep = []
    for i, p in enumerate(probs):
        if p.epi == R.EPI_MASK:
            assert R.mask_margin(p.xprev[:, p.xcol0:p.xcol0 + p.N], p.obn) >= 1e-3
        flat, Y, S = _buffers(p)
        descs[i] = GC.nt_desc(L, p, dev, Y=Y, osums=S)
        keep.append((flat, S))
    grouped = C.c_int(0)
    rc = L.lib().sln_debug_gemm_nt(descs, n, C.byref(grouped), L.current_stream_ptr())
    _sync("sln_debug_gemm_nt under store policy %d" % L.lib().sln_get_store_policy())
    assert rc == 0, rc
    return [(f.cpu(), s.cpu()) for f, s in keep], grouped.value


def _on_against_off(L, probs, dev, policy, tag):
    policy(0)
    off, g0 = _launch(L, probs, dev)
    policy(1)
    on, g1 = _launch(L, probs, dev)
    assert g0 == g1
    for i, p in enumerate(probs):
        (f0, s0), (f1, s1) = off[i], on[i]
        assert torch.equal(f1, f0), "%s[%d]: Y (or a sentinel around it) differs between the policies" % (tag, i)
        assert torch.equal(s1, s0), "%s[%d]: column statistics differ between the policies" % (tag, i)
        Y = f1[1:].view(p.M + 1, p.ldy)
        lo, hi = p.ycol0, p.ycol0 + p.N
        assert f1[0] == SENT and bool((Y[:p.M, :lo] == SENT).all()) and bool((Y[:p.M, hi:] == SENT).all()) and bool((Y[p.M] == SENT).all()), \
            "%s[%d]: a sentinel left of, right of or below the slice was overwritten" % (tag, i)
        ref = R.nt(p)
        rt = GC.route(L, p)
        e, tol = _assert_close(Y[:p.M, lo:hi], ref["y"], 2e-6, 1e-6, "%s[%d] y" % (tag, i), GC.route_text(rt))
        line = "%s[%d] M=%d N=%d K=%d epi=%d ycol0=%d add=%d: y err %.3e bound %.3e" % (tag, i, p.M, p.N, p.K, p.epi, p.ycol0, p.addend is not None, e, tol)
        if ref["sums"] is not None:
            for r in range(2):
                es, ts = _assert_close(s1[r, :p.N], ref["sums"][r], 1e-5, 1e-5, "%s[%d] sum%d" % (tag, i, r), GC.route_text(rt))
                line += " | sum%d err %.3e bound %.3e" % (r, es, ts)
            assert bool((s1[:, p.N:] == SENT).all())
        else:
            assert bool((s1[:, :p.N] == 0).all())
        print(line)
    return g1


def _problem(key, M, N, K, epi, ycol0, with_add, variant, tile=-1):
    # variant % 3 == 0 takes the operand's train-mode BatchNorm statistics over its own M rows (gemm_cases.single_operand): over ONE
    # row the variance is 0, 1 / std is eps ** -0.5 = 316 and fp32 is 3e-5 off the fp64 reference whatever the stores do (torch
    # refuses train-mode BatchNorm over one row).  M = 1 therefore gathers its row from a five-row source, like the odd variants.
    if M == 1 and variant % 3 == 0:
        variant += 1
    p = GC.nt_problem(key, M, N, K, None, MODE_OF_EPI[epi], epi, tile, variant)
    p = p.replace(ycol0=ycol0, ldy=N + ycol0 + 5)
    return p if with_add else p.replace(addend=None)


def _tile(mi, epi):
    """Problems of at most 100 rows all go to the 32 x 32 split-K body when the dispatcher chooses (nt_wants_small); every second
    case asks for the 64 x 64 body instead (the hook's `tile` = 0, as the t64 rows of gemm_cases.NT_SHAPES do)."""
    return 0 if (mi + epi) % 2 else -1


@pytest.mark.parametrize("N", NS)
def test_write_through_gives_the_plain_bits(N, policy):
    L = _lib()
    dev = Dev()
    ni = NS.index(N)
    for mi, M in enumerate(MS):
        for epi in GC.EPIS:
            c = ni + mi + epi
            K, ycol0, with_add = KS[c % 3], YCOL0[(ni + 2 * mi + epi) % 3], (mi + epi + ni) % 2 == 0
            p = _problem("wt-%d-%d-%d" % (M, N, epi), M, N, K, epi, ycol0, with_add, c, _tile(mi, epi))
            _on_against_off(L, [p], dev, policy, "N%d" % N)


@pytest.mark.parametrize("M,N,epi,ycol0,with_add", [(2750, 384, R.EPI_MASK, 4, True), (3330, 640, R.EPI_STATS, 6, False),
                                                   (2750, 384, R.EPI_PLAIN, 0, False), (3330, 640, R.EPI_MASK, 0, True)])
def test_the_16x16_tiles(M, N, epi, ycol0, with_add, policy):
    """Tall problems: the dispatcher takes the 64 x 96 (N = 384) and 64 x 160 (N = 640) tiles of gemm_nt_body16."""
    L = _lib()
    p = _problem("wt16-%d-%d-%d" % (M, N, epi), M, N, 32, epi, ycol0, with_add, epi)
    assert GC.BODY_NAMES[GC.route(L, p)[0]] == ("16x16 J=3" if N == 384 else "16x16 J=5")
    _on_against_off(L, [p], Dev(), policy, "J%d" % (3 if N == 384 else 5))


# the other instantiations that carry the store form: (id, body, MULTI, M, N, K, segment lens, tile) - rows of gemm_cases.NT_SHAPES /
# NT_BIG_SHAPES - each with the three (operand mode, epilogue) forms of gemm_cases.NT_BIG_FORMS
OTHER_BODIES = [s for s in GC.NT_SHAPES if s[0] in ("small3-5x24x384", "small3-64x100x128", "t64m1-200x100x384", "t64m2-133x24x136")] + GC.NT_BIG_SHAPES


@pytest.mark.parametrize("shape", OTHER_BODIES, ids=[s[0] for s in OTHER_BODIES])
def test_the_other_bodies(shape, policy):
    """The three-segment split-K body, the 64 x 64 body with segment boundaries on and inside a k-tile (MULTI 1 and 2) and the
    128 x 64 / 128 x 128 tiles, which the cases above do not reach."""
    L = _lib()
    name, body, multi, M, N, K, lens, tile = shape
    dev = Dev()
    for v, (mode, epi) in enumerate(GC.NT_BIG_FORMS):
        p = GC.nt_problem("wto-%s-%d" % (name, v), M, N, K, lens, mode, epi, tile, v)
        p = p.replace(ycol0=YCOL0[v], ldy=N + YCOL0[v] + 5)
        if v == 1:
            p = p.replace(addend=None)
        rt = GC.route(L, p)
        assert (rt[0], rt[1]) == (body, multi), "%s: route %s" % (name, GC.route_text(rt))
        _on_against_off(L, [p], dev, policy, name)


@pytest.mark.parametrize("key", ["share-affine-stats", "share-ident-plain-multi", "share-bwd-mask"])
def test_grouped_launches(key, policy):
    """One grid for two problems: single-segment operands, a three-segment one (the MULTI form the training step runs) and the
    masked dgrads."""
    L = _lib()
    share, items = GC.NT_GROUPS[key]
    probs = [GC.nt_problem("wtg-%s-%d" % (key, i), M, N, K, lens, mode, epi, -1, i) for i, (M, N, K, lens, mode, epi) in enumerate(items)]
    assert share and _on_against_off(L, probs, Dev(), policy, "grouped") == 1, "the pair must share one grid under both policies"


def test_every_body_is_hit():
    """Host side: the routes of the cases above cover every body of the family - 32 x 32 split-K with one and three segments, 64 x 64
    (one segment, boundaries on and inside a k-tile), 128 x 64, 128 x 128 and both 16 x 16 tiles."""
    L = _lib()
    seen = set()
    for N in NS:
        for mi, M in enumerate(MS):
            for epi in GC.EPIS:
                p = _problem("route-%d-%d" % (M, N), M, N, 32, epi, 0, False, 1, _tile(mi, epi))
                seen.add((N, GC.BODY_NAMES[GC.route(L, p)[0]]))
    for N in NS:
        assert (N, "64x64") in seen and (N, "32x32 split-K 1 seg") in seen, N
    seen = {b for _, b in seen}
    for M, N in ((2750, 384), (3330, 640)):
        seen.add(GC.BODY_NAMES[GC.route(L, _problem("route-%d-%d" % (M, N), M, N, 32, R.EPI_PLAIN, 0, False, 1))[0]])
    seen |= {GC.BODY_NAMES[s[1]] for s in OTHER_BODIES}          # (test_the_other_bodies asserts each of these routes)
    assert seen == set(GC.BODY_NAMES), sorted(set(GC.BODY_NAMES) - seen)
    assert {s[2] for s in OTHER_BODIES if s[1] == GC.B64} == {1, 2}, "both multi-segment forms of the 64 x 64 body"
