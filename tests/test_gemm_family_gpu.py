"""Every body of the fused fp32-MFMA GEMM family (csrc/gemm_f32.hip, gemm_bodies.h, gemm_group.hip) at operand level against the
fp64 reference of tests/gemm_ref.py, through the sln_debug_gemm_* hooks - the engine's own dispatchers with an arbitrary operand.

Tolerances are the family's own (tests/test_vae_gpu.py::test_linear_forward / test_linear_wgrad): rtol 2e-6 / atol 1e-6 on y,
1e-5 on column sums, dW and db, both scaled by the reference's max-abs where that exceeds 1.  Every element is compared; the
masked epilogue's inputs are kept 1e-3 of a column's spread away from its threshold (asserted before the launch) instead.
Each case prints its error, its bound and the error of an fp32 CPU evaluation of the same formulas (gemm_ref with
dtype=float32) - the yardstick for what fp32 arithmetic delivers on a transformed operand."""
import ctypes as C

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
from gpu_util import SENT, Dev, _lib, _sync, _assert_close

pytestmark = pytest.mark.gpu


def _launch_nt(L, probs, dev):
    n = len(probs)
    descs = (L.SlnDbgGemmNT * n)()
    Ys, Ss = [], []
    for i, p in enumerate(probs):
        if p.epi == R.EPI_MASK:          # the cap on elements left out is zero: none may sit on the threshold
            margin = R.mask_margin(p.xprev[:, p.xcol0:p.xcol0 + p.N], p.obn)
            assert margin >= 1e-3, margin
        Y = torch.full((p.M, p.ldy), SENT, device="cuda")
        S = torch.zeros(2, p.ocstride, dtype=torch.float64, device="cuda")
        S[:, p.N:] = SENT
        descs[i] = GC.nt_desc(L, p, dev, Y=Y, osums=S)
        Ys.append(Y); Ss.append(S)
    grouped = C.c_int(0)
    rc = L.lib().sln_debug_gemm_nt(descs, n, C.byref(grouped), L.current_stream_ptr())
    routes = [GC.route_text(GC.route(L, p)) for p in probs]
    _sync("sln_debug_gemm_nt; route: " + " | ".join(routes))
    assert rc == 0, "sln_debug_gemm_nt returned %d; route: %s" % (rc, " | ".join(routes))
    return [Y.cpu() for Y in Ys], [S.cpu() for S in Ss], grouped.value, routes


def _check_nt(p, Y, S, route, tag):
    ref = R.nt(p)
    lo, hi = p.ycol0, p.ycol0 + p.N
    assert bool((Y[:, :lo] == SENT).all()) and bool((Y[:, hi:] == SENT).all()), "%s: wrote outside its column window; route: %s" % (tag, route)
    assert bool((S[:, p.N:] == SENT).all()), "%s: statistics written behind column N; route: %s" % (tag, route)
    e, tol = _assert_close(Y[:, lo:hi], ref["y"], 2e-6, 1e-6, tag + " y", route)
    yard = float((R.nt(p, torch.float32)["y"].double() - ref["y"]).abs().max())
    line = "%s: y err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, yard)
    if ref["sums"] is not None:
        for r, name in enumerate(("sum0", "sum1")):
            es, ts = _assert_close(S[r, :p.N], ref["sums"][r], 1e-5, 1e-5, "%s %s" % (tag, name), route)
            line += " | %s err %.3e bound %.3e" % (name, es, ts)
    else:
        assert bool((S[:, :p.N] == 0).all()), tag + ": EPI_PLAIN touched the statistics"
    print(line)


def _variants(p):
    """with and without bias, with and without an addend"""
    return [("bias+add", p), ("bias", p.replace(addend=None)), ("add", p.replace(bias=None)), ("bare", p.replace(bias=None, addend=None))]


# ----------------------------------------------------------------------------------------------------------------- NT
@pytest.mark.parametrize("case", GC.nt_cases(), ids=GC.nt_case_id)
def test_nt_body(case):
    L = _lib()
    p0 = GC.nt_case_problem(case)
    dev = Dev()
    for name, p in _variants(p0):
        (Y,), (S,), _, (route,) = _launch_nt(L, [p], dev)
        _check_nt(p, Y, S, route, "%s[%s]" % (GC.nt_case_id(case), name))


def _group_problems(key):
    share, items = GC.NT_GROUPS[key]
    probs = [GC.nt_problem("%s-%d" % (key, i), M, N, K, lens, mode, epi, -1, i) for i, (M, N, K, lens, mode, epi) in enumerate(items)]
    return share, probs


@pytest.mark.parametrize("key", sorted(GC.NT_GROUPS))
def test_nt_grouped(key):
    """Two problems in one grid, problem by problem against the reference; pairs that cannot share a kernel take the engine's
    fallback and give the bits of two separate launches."""
    L = _lib()
    share, probs = _group_problems(key)
    dev = Dev()
    Ys, Ss, grouped, routes = _launch_nt(L, probs, dev)
    assert bool(grouped) == share, "grouped launch taken: %d, expected %d" % (grouped, share)
    for i, p in enumerate(probs):
        form = "grouped 64x64" if grouped else routes[i]
        _check_nt(p, Ys[i], Ss[i], form, "%s[%d]" % (key, i))
    if not share:
        for i, p in enumerate(probs):
            (Y,), (S,), _, _ = _launch_nt(L, [p], dev)
            assert torch.equal(Y, Ys[i]), "fallback differs from a separate launch, problem %d" % i
            if p.epi == R.EPI_PLAIN:          # (sums of several workgroups are order-independent by design, but not asserted here)
                assert torch.equal(S, Ss[i])


# ----------------------------------------------------------------------------------------------------------------- TN
def _launch_tn(L, probs, multi, dev):
    n = len(probs)
    descs = (L.SlnDbgGemmTN * n)()
    outs = []
    for i, p in enumerate(probs):
        dW = p.dW0.cuda().clone()
        db = None if p.db0 is None else p.db0.cuda().clone()
        step = None if p.sgd_step is None else torch.tensor([p.sgd_step], dtype=torch.float32, device="cuda")
        descs[i] = GC.tn_desc(L, p, dev, dW, db, step)
        outs.append((dW, db, step))
    rc = L.lib().sln_debug_gemm_tn(descs, n, 1 if multi else 0, L.current_stream_ptr())
    _sync("sln_debug_gemm_tn; " + " | ".join(_tn_form(p) for p in probs))
    assert rc == 0, "sln_debug_gemm_tn returned %d (%s)" % (rc, "per-pass launch" if multi else "single launch")
    return [(dW.cpu(), None if db is None else db.cpu()) for dW, db, _ in outs]


def _tn_form(p):
    return "gemm_tn G_X2=%d XG=%d" % (any(s.x2 is not None for s in p.G.segs), any(s.which for s in p.X.segs))


def _check_tn(p, dW, db, tag):
    rW, rb = R.tn(p)
    form = _tn_form(p)
    assert torch.equal(dW[:, p.Kin:], p.dW0[:, p.Kin:]), "%s: wrote behind column Kin; %s" % (tag, form)
    e, tol = _assert_close(dW[:, :p.Kin], rW, 1e-5, 1e-5, tag + " dW", form)
    yW, yb = R.tn(p, torch.float32)
    line = "%s: dW err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, float((yW.double() - rW).abs().max()))
    if rb is not None:
        eb, tb = _assert_close(db, rb, 1e-5, 1e-5, tag + " db", form)
        line += " | db err %.3e bound %.3e fp32-yardstick %.3e" % (eb, tb, float((yb.double() - rb).abs().max()))
    print(line)


@pytest.mark.parametrize("case", GC.tn_cases(), ids=GC.tn_case_id)
def test_tn_body(case):
    """The four G_X2 x XG forms, += onto non-zero dW / db, with and without db."""
    L = _lib()
    (Rr, Nout, Kin), gf, xf = case
    p = GC.tn_problem(GC.tn_case_id(case), Rr, Nout, Kin, gf, xf)
    dev = Dev()
    for name, q in (("db", p), ("nodb", p.replace(db0=None))):
        ((dW, db),) = _launch_tn(L, [q], False, dev)
        _check_tn(q, dW, db, "%s[%s]" % (GC.tn_case_id(case), name))


@pytest.mark.parametrize("case", [((1000, 100, 256), "bwd", "concat"), ((300, 24, 100), "plain", "relu"), ((13, 8, 36), "plain", "ident")],
                         ids=GC.tn_case_id)
@pytest.mark.parametrize("multi", [False, True], ids=["single", "perpass"])
def test_tn_sgd_epilogue(case, multi):
    """With sgd_step the buffers are the parameters: param - step * grad."""
    L = _lib()
    (Rr, Nout, Kin), gf, xf = case
    p = GC.tn_problem("sgd-" + GC.tn_case_id(case), Rr, Nout, Kin, gf, xf, sgd_step=0.0625 + 1.0 / 3.0)
    ((dW, db),) = _launch_tn(L, [p], multi, Dev())
    _check_tn(p, dW, db, "sgd-%s[%s]" % (GC.tn_case_id(case), "perpass" if multi else "single"))


def _multi_problems(key):
    return [GC.tn_problem("%s-%d" % (key, i), Rr, Nout, Kin, gf, xf, with_db=(i % 2 == 0))
            for i, (Rr, Nout, Kin, gf, xf) in enumerate(GC.TN_MULTI[key])]


@pytest.mark.parametrize("key", sorted(GC.TN_MULTI))
def test_tn_multi(key):
    """Every wgrad of a pass in one launch off a device-side table; the same again with one chunk per problem (deterministic
    mode): two runs bit-identical, and within tolerance of the reference and hence of the default mode."""
    L = _lib()
    probs = _multi_problems(key)
    dev = Dev()
    outs = _launch_tn(L, probs, True, dev)
    for i, p in enumerate(probs):
        _check_tn(p, outs[i][0], outs[i][1], "%s[%d]" % (key, i))
    was = L.lib().sln_get_deterministic()
    try:
        L.lib().sln_set_deterministic(1)
        d1 = _launch_tn(L, probs, True, dev)
        d2 = _launch_tn(L, probs, True, dev)
    finally:
        L.lib().sln_set_deterministic(was)
    for i, p in enumerate(probs):
        assert torch.equal(d1[i][0], d2[i][0]), "%s[%d]: dW differs between two deterministic runs" % (key, i)
        assert (d1[i][1] is None) or torch.equal(d1[i][1], d2[i][1]), "%s[%d]: db differs between two deterministic runs" % (key, i)
        _check_tn(p, d1[i][0], d1[i][1], "%s[%d] deterministic" % (key, i))
        form = _tn_form(p)
        _assert_close(d1[i][0][:, :p.Kin], outs[i][0][:, :p.Kin], 2e-5, 2e-5, "%s[%d] deterministic vs default dW" % (key, i), form)
        if p.db0 is not None:
            _assert_close(d1[i][1], outs[i][1], 2e-5, 2e-5, "%s[%d] deterministic vs default db" % (key, i), form)


def test_hooks_refuse_bad_descriptions_without_launching():
    L = _lib()
    p = GC.nt_problem("refuse", 70, 100, 36, None, "ident", R.EPI_PLAIN, -1, 0)
    dev = Dev()
    Y = torch.full((p.M, p.ldy), SENT, device="cuda")
    S = torch.zeros(2, p.ocstride, dtype=torch.float64, device="cuda")
    d = GC.nt_desc(L, p, dev, Y=Y, osums=S)
    d.K = 40
    assert L.lib().sln_debug_gemm_nt(C.byref(d), 1, None, L.current_stream_ptr()) == -1
    t = GC.tn_problem("refuse-tn", 13, 8, 36, "plain", "ident")
    dW = t.dW0.cuda().clone()
    dt = GC.tn_desc(L, t, dev, dW, None, None)
    dt.G.seg[0].which = 1
    assert L.lib().sln_debug_gemm_tn(C.byref(dt), 1, 0, L.current_stream_ptr()) == -1
    assert L.lib().sln_debug_gemm_tn(C.byref(dt), 2, 0, L.current_stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((Y == SENT).all()) and torch.equal(dW.cpu(), t.dW0)
