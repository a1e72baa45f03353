"""Case table of the GEMM-family suite and the bridge from a gemm_ref problem to the C descriptions of the test hooks.

Shared by tests/test_gemm_ref_host.py (routes, struct layout; no GPU) and tests/test_gemm_family_gpu.py.  Inputs: operands ~N(0, 1),
weights scaled by 1 / sqrt(K), gamma in [0.5, 1.5], running variances in [0.5, 2].  Leading dimensions are wider than the logical
widths and first columns are non-zero wherever the kernels allow it (multiples of 4: rows are read as float4)."""
import ctypes as C

import torch

import gemm_ref as R

# body ids of SlnDbgNTRoute
B64, B128x64, B128, B16J3, B16J5, BSMALL, BSMALL3 = range(7)
BODY_NAMES = ["64x64", "128x64", "128x128", "16x16 J=3", "16x16 J=5", "32x32 split-K 1 seg", "32x32 split-K 3 seg"]
MODES = ("ident", "affine", "bwd")          # operand modes 2, 0, 1 of the kernels
AMODE_OF = {"ident": 2, "affine": 0, "bwd": 1}
EPIS = (R.EPI_PLAIN, R.EPI_STATS, R.EPI_MASK)
EPI_NAMES = ["plain", "stats", "mask"]


def _seed(*key):      # hash() of str is salted per process: spell the seed out
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _uniform(g, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=g)


def gather_index(g, n, src_rows):
    """n row ids below src_rows: a non-monotone permutation, cycled, with a repeat."""
    perm = torch.randperm(src_rows, generator=g)
    idx = perm[torch.arange(n) % src_rows].clone()
    if n > 1:
        idx[1] = idx[0]
    if n > 3:
        idx[n - 1] = idx[n // 2]
    return idx.to(torch.int32)


def bn_train(g, x):
    """Train-mode view over ALL rows of x (the statistics run over the source's rows, not over the gathered ones)."""
    c = x.shape[1]
    return R.Bn(mode=R.BN_TRAIN, gamma=_uniform(g, c, 0.5, 1.5), beta=0.5 * _randn(g, c), sums=R.sums_of(x), n_rows=float(x.shape[0]))


def bn_eval(g, c):
    return R.Bn(mode=R.BN_EVAL, gamma=_uniform(g, c, 0.5, 1.5), beta=0.5 * _randn(g, c), rmean=0.3 * _randn(g, c),
                rvar=_uniform(g, c, 0.5, 2.0))


def bn_train_bwd(g, grad, pre):
    """View for SLN_COEF_BWD: forward statistics of the pre-activation, backward sums of (grad, grad * xhat), over all rows."""
    bn = bn_train(g, pre)
    mean, istd = R.mean_istd(bn, pre.shape[1], torch.float64)
    gd = grad.double()
    bn.gsums = torch.stack([gd.sum(0), (gd * ((pre.double() - mean) * istd)).sum(0)])
    return bn


def _seg(g, rows, length, mode, variant, which, c1=4):
    """One segment of `length` columns over a fresh source of `rows` rows."""
    x1 = _randn(g, rows, length + c1 + 4)
    view = x1[:, c1:c1 + length]
    if mode == "ident":
        return R.Seg(x1=x1, c1=c1, len=length, which=which, coef=R.COEF_IDENT)
    if mode == "affine":
        x1 = x1 + 0.5          # a mean next to the spread, as pre-activations have
        view = x1[:, c1:c1 + length]
        coef = R.COEF_FWD if variant % 2 == 0 else R.COEF_FWD_NORELU
        bn = bn_eval(g, length) if variant % 3 == 2 else bn_train(g, view)
        return R.Seg(x1=x1, c1=c1, len=length, which=which, coef=coef, bn=bn)
    x2 = _randn(g, rows, length + 8) + 0.5
    c2 = 8
    return R.Seg(x1=x1, c1=c1, x2=x2, c2=c2, len=length, which=which, coef=R.COEF_BWD, bn=bn_train_bwd(g, view, x2[:, c2:c2 + length]))


def single_operand(g, M, K, mode, variant):
    which = 0 if M == 8 else variant % 3          # M = 8: statistics over the 8 rows themselves (the quantum rule's case)
    rows = M if which == 0 else max(5, M // 2 + 3)
    seg = _seg(g, rows, K, mode, 0 if M == 8 else variant, which)
    ia = gather_index(g, M, rows) if which else None
    ib = gather_index(g, M, rows) if which else None
    return R.Operand(segs=(seg,), idx_a=ia, idx_b=ib)


def concat_operand(g, M, lens, mode, variant):
    """GraphTripleConv's [obj[s] | pred | obj[o]] (three lens) or box_net's [obj_vecs | attr_emb[attrs]] (two lens)."""
    n_obj = max(5, M // 2 + 3)
    ia, ib = gather_index(g, M, n_obj), gather_index(g, M, n_obj)
    if len(lens) == 2:
        segs = (_seg(g, M, lens[0], mode if mode != "bwd" else "ident", variant, 0),
                _seg(g, n_obj, lens[1], mode, variant + 1, 1 + variant % 2))
        return R.Operand(segs=segs, idx_a=ia, idx_b=ib)
    side = "ident" if mode == "bwd" else mode          # two-source: the middle segment alone carries a second source
    s0 = _seg(g, n_obj, lens[0], side, 0 if mode == "affine" else variant, 1, c1=0)
    s1 = _seg(g, M, lens[1], mode, 0 if (mode == "affine" and variant % 2 == 0) else variant, 0)
    s2 = _seg(g, n_obj, lens[2], side, 0 if mode == "affine" else variant, 2, c1=0)
    return R.Operand(segs=(s0, s1, s2), idx_a=ia, idx_b=ib)


def nt_problem(key, M, N, K, lens, mode, epi, tile, variant):
    """A full NT problem: bias and addend present (the tests also run it without either)."""
    g = _seed(key)
    A = single_operand(g, M, K, mode, variant) if lens is None else concat_operand(g, M, lens, mode, variant)
    W = _randn(g, N, K + 4) / K ** 0.5
    ycol0 = 3
    p = R.NT(A=A, W=W, bias=_randn(g, N), M=M, N=N, K=K, ldy=N + ycol0 + 5, ycol0=ycol0, addend=_randn(g, M, N + 6), addcol0=2,
             epi=epi, tile=tile, ocstride=N + 3)
    if epi == R.EPI_MASK:
        xcol0 = 1
        xp = _randn(g, M, N + 3) + 0.25
        if variant % 2 == 0:
            gamma, beta = _uniform(g, N, 0.5, 1.5), 0.5 * _randn(g, N)

            def make(x):
                return R.Bn(mode=R.BN_TRAIN, gamma=gamma, beta=beta, sums=R.sums_of(x), n_rows=float(M))
        else:
            fixed = bn_eval(g, N)

            def make(x):
                return fixed
        xv, obn = R.condition_mask(xp[:, xcol0:xcol0 + N], make)
        xp[:, xcol0:xcol0 + N] = xv
        p.xprev, p.xcol0, p.obn = xp, xcol0, obn
    return p


# ------------------------------------------------------------------------------------------------ the NT table
# (id, expected body, expected MULTI form, M, N, K, segment lens or None, tile)
NT_SHAPES = [
    ("small-8x6x36", BSMALL, 0, 8, 6, 36, None, -1),
    ("small-70x100x256", BSMALL, 0, 70, 100, 256, None, -1),
    ("small-33x24x640", BSMALL, 0, 33, 24, 640, None, -1),
    ("small3-5x24x384", BSMALL3, 1, 5, 24, 384, (128, 128, 128), -1),
    ("small3-64x100x128", BSMALL3, 1, 64, 100, 128, (32, 64, 32), -1),
    ("t64-70x100x36", B64, 0, 70, 100, 36, None, 0),
    ("t64-133x6x100", B64, 0, 133, 6, 100, None, 0),
    ("t64m1-200x100x384", B64, 1, 200, 100, 384, (128, 128, 128), -1),
    ("t64m2-133x24x136", B64, 2, 133, 24, 136, (36, 100), -1),
    ("j3-2750x380x36", B16J3, 0, 2750, 380, 36, None, -1),
    ("j5-3330x636x36", B16J5, 0, 3330, 636, 36, None, -1),
]
# the two big tiles: a thinner set of (mode, epilogue)
NT_BIG_SHAPES = [
    ("t128x64-133x100x100", B128x64, 0, 133, 100, 100, None, 1),
    ("t128x64m1-260x136x384", B128x64, 1, 260, 136, 384, (128, 128, 128), 1),
    ("t128-133x100x100", B128, 0, 133, 100, 100, None, 2),
    ("t128m1-260x136x384", B128, 1, 260, 136, 384, (128, 128, 128), 2),
]
NT_BIG_FORMS = [("ident", R.EPI_PLAIN), ("affine", R.EPI_STATS), ("bwd", R.EPI_MASK)]


def nt_cases():
    out = []
    for shp in NT_SHAPES:
        v = 0
        for mode in MODES:
            for epi in EPIS:
                out.append((shp, mode, epi, v))
                v += 1
    for shp in NT_BIG_SHAPES:
        for v, (mode, epi) in enumerate(NT_BIG_FORMS):
            out.append((shp, mode, epi, v))
    return out


def nt_case_id(c):
    shp, mode, epi, _ = c
    return "%s-%s-%s" % (shp[0], mode, EPI_NAMES[epi])


def nt_case_problem(c):
    (name, _, _, M, N, K, lens, tile), mode, epi, v = c
    return nt_problem(nt_case_id(c), M, N, K, lens, mode, epi, tile, v)


# ------------------------------------------------------------------------------------------------ TN
TN_SHAPES = [(13, 8, 36), (300, 24, 100), (1000, 100, 256)]
TN_G = ("plain", "bwd")
TN_X = ("ident", "relu", "concat")
TN_CONCAT_LENS = {36: (32, 4), 100: (32, 32, 36), 256: (96, 64, 96)}


def tn_problem(key, Rr, Nout, Kin, gform, xform, with_db=True, sgd_step=None):
    g = _seed(key)
    gseg = _seg(g, Rr, Nout, "bwd" if gform == "bwd" else "ident", 0, 0)
    G = R.Operand(segs=(gseg,))
    if xform == "concat":
        lens = TN_CONCAT_LENS[Kin]
        n_obj = max(5, Rr // 2 + 3)
        ia, ib = gather_index(g, Rr, n_obj), gather_index(g, Rr, n_obj)
        if len(lens) == 2:
            segs = (_seg(g, n_obj, lens[0], "affine", 0, 1), _seg(g, n_obj, lens[1], "ident", 0, 2))
        else:
            segs = (_seg(g, n_obj, lens[0], "affine", 0, 1, c1=0), _seg(g, Rr, lens[1], "affine", 2, 0),
                    _seg(g, n_obj, lens[2], "ident", 0, 2, c1=0))
        X = R.Operand(segs=segs, idx_a=ia, idx_b=ib)
    else:
        X = R.Operand(segs=(_seg(g, Rr, Kin, "affine" if xform == "relu" else "ident", 0, 0),))
    return R.TN(G=G, X=X, R=Rr, Nout=Nout, Kin=Kin, dW0=_randn(g, Nout, Kin + 4), db0=_randn(g, Nout) if with_db else None,
                sgd_step=sgd_step)


def tn_cases():
    return [(s, gf, xf) for s in TN_SHAPES for gf in TN_G for xf in TN_X]


def tn_case_id(c):
    return "%dx%dx%d-%s-%s" % (c[0] + (c[1], c[2]))


# problems of the per-pass launch: (R, Nout, Kin, G form, X form)
TN_MULTI = {
    "n1-plain": [(300, 24, 100, "plain", "ident")],
    "n1-gather-x2": [(1000, 100, 256, "bwd", "concat")],
    "n2-gather+plain": [(300, 24, 100, "plain", "concat"), (13, 8, 36, "plain", "relu")],
    "n2-x2+plain": [(1000, 100, 256, "bwd", "ident"), (300, 24, 100, "plain", "relu")],
    "n5-mixed": [(1000, 100, 256, "plain", "concat"), (13, 8, 36, "bwd", "ident"), (300, 24, 100, "plain", "relu"),
                 (2100, 24, 36, "plain", "concat"), (70, 100, 100, "bwd", "relu")],
}

# grouped NT launches: two problems (M, N, K, lens, mode, epi)
NT_GROUPS = {
    "share-affine-stats": (True, [(70, 100, 36, None, "affine", R.EPI_STATS), (133, 24, 100, None, "affine", R.EPI_STATS)]),
    "share-ident-plain-multi": (True, [(200, 100, 384, (128, 128, 128), "ident", R.EPI_PLAIN), (70, 6, 36, None, "ident", R.EPI_PLAIN)]),
    "share-bwd-mask": (True, [(133, 24, 100, None, "bwd", R.EPI_MASK), (70, 100, 256, None, "bwd", R.EPI_MASK)]),
    "fallback-modes": (False, [(70, 100, 36, None, "affine", R.EPI_PLAIN), (133, 24, 100, None, "ident", R.EPI_PLAIN)]),
    "fallback-unaligned": (False, [(133, 24, 136, (36, 100), "ident", R.EPI_PLAIN), (70, 100, 36, None, "ident", R.EPI_PLAIN)]),
}


# ------------------------------------------------------------------------------------------------ bounds, C descriptions
def _check_operand(op, rows, cols):
    assert 1 <= len(op.segs) <= 3
    tot = 0
    for s in op.segs:
        need = rows
        if s.which:
            idx = op.idx_a if s.which == 1 else op.idx_b
            assert idx is not None and idx.dtype == torch.int32 and idx.numel() >= rows
            assert int(idx.min()) >= 0
            need = int(idx.max()) + 1
        for x, c in ((s.x1, s.c1), (s.x2, s.c2)):
            if x is not None:
                assert x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] >= need and x.shape[1] >= c + s.len
                assert x.shape[1] % 4 == 0 and c % 4 == 0
        if s.bn is not None and s.coef != R.COEF_IDENT:
            for t in (s.bn.gamma, s.bn.beta, s.bn.rmean, s.bn.rvar):
                assert t is None or (t.dtype == torch.float32 and t.numel() >= s.len)
            for t in (s.bn.sums, s.bn.gsums):
                assert t is None or (t.dtype == torch.float64 and t.shape[0] == 2 and t.shape[1] >= s.len and t.is_contiguous())
        tot += s.len
    assert tot == cols


def check_nt(p):
    """Every address a kernel may form stays inside its tensor (the kernels clamp rows to M - 1 and columns to the widths)."""
    _check_operand(p.A, p.M, p.K)
    assert p.W.shape[0] >= p.N and p.W.shape[1] >= p.K and p.W.shape[1] % 4 == 0
    assert p.bias is None or p.bias.numel() >= p.N
    assert p.ldy >= p.ycol0 + p.N
    assert p.addend is None or (p.addend.shape[0] >= p.M and p.addend.shape[1] >= p.addcol0 + p.N)
    if p.epi == R.EPI_MASK:
        assert p.xprev.shape[0] >= p.M and p.xprev.shape[1] >= p.xcol0 + p.N
        for t in (p.obn.gamma, p.obn.beta, p.obn.rmean, p.obn.rvar):
            assert t is None or t.numel() >= p.N
        assert p.obn.sums is None or p.obn.sums.shape[1] >= p.N
    assert p.ocstride >= p.N


def check_tn(p):
    _check_operand(p.G, p.R, p.Nout)
    _check_operand(p.X, p.R, p.Kin)
    assert all(s.which == 0 for s in p.G.segs)
    assert p.dW0.shape[0] >= p.Nout and p.dW0.shape[1] >= p.Kin
    assert p.db0 is None or p.db0.numel() >= p.Nout


def _bn_desc(L, bn, ptr):
    d = L.SlnDbgBn()
    if bn is None:
        d.n_rows, d.eps = 1.0, 1e-5
        return d
    for n in ("sums", "gsums", "gamma", "beta", "rmean", "rvar"):
        setattr(d, n, ptr(getattr(bn, n)))
    d.cstride = 0 if bn.sums is None else bn.sums.shape[1]
    if bn.gsums is not None:
        assert bn.sums is not None and bn.gsums.shape[1] == bn.sums.shape[1]
    d.mode, d.n_rows, d.eps = bn.mode, bn.n_rows, bn.eps
    return d


def _operand_desc(L, op, ptr):
    d = L.SlnDbgOperand()
    for i, s in enumerate(op.segs):
        g = d.seg[i]
        g.x1, g.x2 = ptr(s.x1), ptr(s.x2)
        g.ld1, g.ld2 = s.x1.shape[1], 0 if s.x2 is None else s.x2.shape[1]
        g.c1, g.c2, g.len, g.which, g.coef = s.c1, s.c2, s.len, s.which, s.coef
        g.bn = _bn_desc(L, s.bn, ptr)
    d.idx_a, d.idx_b, d.nseg = ptr(op.idx_a), ptr(op.idx_b), len(op.segs)
    return d


def nt_desc(L, p, ptr, Y=None, osums=None):
    """ptr(tensor or None) -> address; Y / osums: the output buffers (any objects ptr understands)."""
    check_nt(p)
    d = L.SlnDbgGemmNT()
    d.A = _operand_desc(L, p.A, ptr)
    d.W, d.bias, d.Y, d.addend, d.xprev = ptr(p.W), ptr(p.bias), ptr(Y), ptr(p.addend), ptr(p.xprev)
    if p.epi == R.EPI_STATS:
        d.osums = ptr(osums)
    if p.epi == R.EPI_MASK:
        d.ogsums = ptr(osums)
    d.obn = _bn_desc(L, p.obn if p.epi == R.EPI_MASK else None, ptr)
    d.M, d.N, d.K, d.ldw, d.ldy, d.ycol0 = p.M, p.N, p.K, p.W.shape[1], p.ldy, p.ycol0
    d.ldadd, d.addcol0 = (0, 0) if p.addend is None else (p.addend.shape[1], p.addcol0)
    d.ldx, d.xcol0 = (0, 0) if p.xprev is None else (p.xprev.shape[1], p.xcol0)
    d.ocstride, d.epi, d.tile = p.ocstride, p.epi, p.tile
    return d


def tn_desc(L, p, ptr, dW, db, step):
    check_tn(p)
    d = L.SlnDbgGemmTN()
    d.G, d.X = _operand_desc(L, p.G, ptr), _operand_desc(L, p.X, ptr)
    d.dW, d.db, d.sgd_step = ptr(dW), ptr(db), ptr(step)
    d.lddw, d.R, d.Nout, d.Kin, d.rows_per_block = p.dW0.shape[1], p.R, p.Nout, p.Kin, p.rows_per_block
    return d


def fake_ptr(t):
    """Host-only hooks never follow a pointer: any aligned non-null address stands for a present tensor."""
    return None if t is None else 4096


def route(L, p):
    d = nt_desc(L, p, fake_ptr, Y=1, osums=1)
    r = L.SlnDbgNTRoute()
    rc = L.lib().sln_debug_gemm_nt_route(C.byref(d), C.byref(r))
    assert rc == 0, "sln_debug_gemm_nt_route: %d" % rc
    return r.body, r.multi, r.amode, r.threads


def route_text(rt):
    return "body %s, MULTI %d, operand mode %d, %d threads" % (BODY_NAMES[rt[0]], rt[1], rt[2], rt[3])
