"""The non-GEMM kernels of the VAE path (csrc/vae_kernels.hip) one by one against the fp64 reference of tests/vae_ref.py, through
the sln_debug_vae_* hooks - the engine's own launchers on caller-built operands.

Every output element is compared.  Everything a kernel may write and what lies beside it (columns behind the logical width, one
row behind the last, statistics behind C, dst_ld / ld_dbp padding) is prefilled with SENT and must come back untouched; `+=`
outputs start from non-zero values.  ReLU masks: the pre-activation is drawn with condition_mask and mask_margin >= 1e-3 is
asserted before the launch, so no element is left out.  Tolerances are the project's own: rtol 2e-6 / atol 1e-6 on values, 1e-5
on column statistics and accumulated tables, both scaled by the reference's max-abs above 1; integer outputs, copies,
transposes and zeroing are exact.  Each case prints its error, its bound and the error of an fp32 CPU evaluation of the same
formulas (vae_ref with dtype=float32).

Train-mode BatchNorm over ONE row is left to the eval / none views: its variance is 0, 1/std = 316, and scale * x + shift
cancels to beta with an fp32 error of 316 |x| 2^-24 - a mask flip there is arithmetic, not a kernel fault.

Covered here: CSR build, the four edge kernels with their room-table forms, bn_relu_apply, add2, loss, log_softmax (+ backward),
latent_bwd, bn_running_update, bn_param_grads, transpose_table, Adam, the Philox draw, the embedding group (assembly and its
gradients through the LDS, plain-atomic and deterministic routes, gathers, id staging and checks) with its room-table forms, and
the one-launch step prologue against the launches it replaces.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_cases as GC
import vae_ref as V
from gpu_util import SENT, _lib, _sync, _assert_close

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
BASE = 0.25            # what `+=` statistics start from (a multiple of every quantum of sln_common.h: added exactly)


def _cu(t):
    return t.contiguous().cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _yard(f, *a, **k):
    """max distance of the fp32 evaluation of a reference function from its fp64 evaluation"""
    r64, r32 = f(*a, dtype=F64, **k), f(*a, dtype=F32, **k)
    if not isinstance(r64, tuple):
        r64, r32 = (r64,), (r32,)
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(r64, r32) if x is not None and x.numel())


def _untouched(t, what):
    assert bool((t == SENT).all()), what + " was written"


# ================================================================================================= graphs
def ladder_graph(degs, seed, num_preds=5):
    """Rows 0 .. len(degs) - 1 get exactly these degrees (self-loops and edges in both directions); one more row, the sink,
    takes the other ends - the long row of the graph.  -> (triples int64 [T, 3], O)"""
    g = GC._seed("ladder", seed, *degs)
    O, sink, ed = len(degs) + 1, len(degs), []
    for i, d in enumerate(degs):
        ns = d // 4
        ed += [(i, i)] * ns
        ed += [(i, sink) if k % 2 == 0 else (sink, i) for k in range(d - 2 * ns)]
    T = len(ed)
    tri = torch.zeros(T, 3, dtype=torch.int64)
    if T:
        e = torch.tensor(ed, dtype=torch.int64)[torch.randperm(T, generator=g)]
        tri[:, 0], tri[:, 2], tri[:, 1] = e[:, 0], e[:, 1], torch.randint(0, num_preds, (T,), generator=g)
    return tri, O


def loops_graph(T):
    """O = 1: T self-loops, degree 2 T, entries e and e + T in the one row"""
    return torch.zeros(T, 3, dtype=torch.int64), 1


def random_graph(T, O, seed):
    g = GC._seed("random-graph", T, O, seed)
    tri = torch.randint(0, O, (T, 3), generator=g)
    tri[:, 1] = 0
    return tri, O


LADDER9 = [0, 1, 2, 16, 17, 64, 65, 80]
GRAPHS = {1: lambda: loops_graph(33), 5: lambda: ladder_graph([17, 64, 65, 0], 5), 9: lambda: ladder_graph(LADDER9, 9),
          17: lambda: ladder_graph(LADDER9 + [3] * 8, 17)}


class HostCsr:
    """The CSR arrays built on the host (vae_ref.csr) and uploaded: the edge tests do not lean on the CSR kernels."""

    def __init__(self, L, tri, O):
        self.ref = r = V.csr(tri, O, 1 << 30)
        self.T, self.O = tri.shape[0], O
        self.s, self.o = r["s"].long(), r["o"].long()
        ent = torch.tensor([e for row in r["rows"] for e in row], dtype=torch.int32)
        self.t = dict(s=_cu(r["s"]), p=_cu(r["p"]), o=_cu(r["o"]), deg=_cu(r["deg"]), invdeg=_cu(1.0 / r["deg"].clamp_min(1).float()),
                      rowptr=_cu(r["rowptr"].int()), cursor=torch.zeros(O, dtype=torch.int32, device="cuda"), ent=_cu(ent))
        self.desc = csr_desc(L, self.t, self.T, O)


def csr_desc(L, t, T, O):
    d = L.SlnDbgCsr()
    for k, v in t.items():
        setattr(d, k, _p(v))
    d.T, d.O = T, O
    return d


# ================================================================================================= BatchNorm views
class Keep:
    """device copies of a view's tensors, kept alive for the launch"""

    def __init__(self):
        self.m = []

    def __call__(self, t):
        if t is None:
            return None
        self.m.append(_cu(t))
        return self.m[-1].data_ptr()


def pad_sums(bn, extra=3):
    """cstride > C: columns behind C hold a value that would wreck any coefficient computed from them"""
    if bn is not None and bn.sums is not None:
        bn.sums = torch.cat([bn.sums, torch.full((2, extra), 1e30, dtype=F64)], 1).contiguous()
    return bn


def make_bn(mode, g, x):
    if mode == "none":
        return None
    return pad_sums(GC.bn_train(g, x)) if mode == "train" else GC.bn_eval(g, x.shape[1])


def masked_input(mode, g, x):
    """-> (x moved off the mask threshold, its view); the margin is asserted: no element is left out of any comparison"""
    if mode == "none":
        x = torch.where(x.abs() < 1e-2, torch.full_like(x, 0.05), x)
        assert float(x.abs().min()) >= 1e-3
        return x, None
    if mode == "eval":
        bn0 = GC.bn_eval(g, x.shape[1])
        x, bn = V.condition_mask(x, lambda _x: bn0)
    else:
        gamma, beta = GC._uniform(g, x.shape[1], 0.5, 1.5), 0.5 * GC._randn(g, x.shape[1])
        x, bn = V.condition_mask(x, lambda _x: V.Bn(mode=V.BN_TRAIN, gamma=gamma, beta=beta, sums=V.sums_of(_x), n_rows=float(_x.shape[0])))
    m = V.mask_margin(x, bn)
    assert m >= 1e-3, m
    return x, pad_sums(bn)


def gsums_buf(C_, extra=3):
    s = torch.full((2, C_ + extra), SENT, dtype=F64, device="cuda")
    s[:, :C_] = BASE
    return s


def check_gsums(S, ref, C_, tag, form):
    S = S.cpu()
    _untouched(S[:, C_:], tag + ": statistics behind column C")
    out = []
    for r in range(2):
        out.append(_assert_close(S[r, :C_] - BASE, ref[r], 1e-5, 1e-5, "%s gsums[%d]" % (tag, r), form))
    return " | gsums err %.3e %.3e bound %.3e %.3e" % (out[0][0], out[1][0], out[0][1], out[1][1])


# ================================================================================================= edge launches
K_SCATTER_FWD, K_SCATTER_BWD, K_GATHER_BWD, K_MASK_GSTATS, K_BN_RELU, K_ADD2 = range(6)


def edge_desc(L, kind, keep, g=None, bn=None, a=None, b=None, c=None, out=None, gsums=None, **ints):
    d = L.SlnDbgEdge()
    d.kind = kind
    if g is not None:
        d.g = g.desc
    d.bn = GC._bn_desc(L, bn, keep)
    d.a, d.b, d.c, d.out, d.gsums = _p(a), _p(b), _p(c), _p(out), _p(gsums)
    keep.m += [a, b, c, out, gsums]
    for k, v in ints.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def launch_edge(L, descs, multi=0, what="edge"):
    arr = (L.SlnDbgEdge * len(descs))(*descs)
    var = C.c_int(-9)
    rc = L.lib().sln_debug_vae_edge(arr, len(descs), multi, C.byref(var), L.current_stream_ptr())
    _sync("sln_debug_vae_edge " + what)
    return rc, var.value


def scatter_fwd_problem(L, H, D, bnmode, gkey, seed=0):
    tri, O = GRAPHS[gkey]()
    csr = HostCsr(L, tri, O)
    g = GC._seed("scatter-fwd", H, D, bnmode, gkey, seed)
    Cc, ld = 2 * H + D, 2 * H + D + 4
    A2 = GC._randn(g, csr.T, ld)
    bn = make_bn(bnmode, g, A2[:, :Cc].contiguous())
    return dict(csr=csr, A2=A2, bn=bn, H=H, D=D, ld=ld, O=O)


def scatter_fwd_launch(L, p, multi_with=None):
    """-> pooled [O + 1, H] (row O is the guard) of a single-room launch"""
    keep = Keep()
    out = torch.full((p["O"] + 1, p["H"]), SENT, device="cuda")
    d = edge_desc(L, K_SCATTER_FWD, keep, g=p["csr"], bn=p["bn"], a=_cu(p["A2"]), out=out, lda=p["ld"], H=p["H"], D=p["D"], rows=p["O"])
    keep.m.append(d)
    return d, out, keep


def scatter_fwd_check(p, out, tag, form):
    out = out.cpu()
    _untouched(out[p["O"]:], tag + ": the row behind O")
    a = (p["A2"], p["H"], p["D"], p["bn"], p["csr"].s, p["csr"].o, p["O"])
    e, tol = _assert_close(out[:p["O"]], V.scatter_avg_fwd(*a), 2e-6, 1e-6, tag, form)
    print("%s: err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, _yard(V.scatter_avg_fwd, *a)))


@pytest.mark.parametrize("bnmode", ["none", "train", "eval"])
@pytest.mark.parametrize("H", [4, 128, 132, 260])
def test_scatter_avg_fwd(H, bnmode):
    """Both variants (H <= 128: 32 x 8, above: 64 x 4), a second column block (132 over 128, 260 over 256), O no multiple of the
    row lanes, rows of degree 0 .. 80 and a sink above 200: 16 / 17 straddle the entries in flight, 64 / 65 the LDS entry cache."""
    L = _lib()
    for D in (4, 8):
        for gkey in (1, 5, 9):
            p = scatter_fwd_problem(L, H, D, bnmode, gkey)
            d, out, keep = scatter_fwd_launch(L, p)
            rc, var = launch_edge(L, [d], what="scatter_avg_fwd H=%d" % H)
            assert rc == 0 and var == -1, rc
            scatter_fwd_check(p, out, "scatter_fwd[H=%d D=%d O=%d %s]" % (H, D, p["O"], bnmode), "64x4" if H > 128 else "32x8")


def test_scatter_avg_fwd_refuses_a_width_that_is_no_multiple_of_four():
    L = _lib()
    p = scatter_fwd_problem(L, 6, 4, "none", 5)
    d, out, keep = scatter_fwd_launch(L, p)
    rc, _ = launch_edge(L, [d], what="scatter_avg_fwd H=6")
    assert rc == -2
    _untouched(out.cpu(), "pooled of a refused launch")


def scatter_bwd_problem(L, T, H, D, bnmode, with_dp, seed=0):
    tri, O = random_graph(T, 5, seed)
    csr = HostCsr(L, tri, O)
    g = GC._seed("scatter-bwd", T, H, D, bnmode, with_dp, seed)
    Cc, ld = 2 * H + D, 2 * H + D + 4
    x, bn = masked_input(bnmode, g, GC._randn(g, T, Cc))
    A2 = torch.cat([x, GC._randn(g, T, ld - Cc)], 1).contiguous()
    dP = GC._randn(g, T, D + 12) if with_dp else None
    return dict(csr=csr, A2=A2, bn=bn, H=H, D=D, ld=ld, T=T, O=O, dM=GC._randn(g, O, H), dP=dP, dpcol0=8 if with_dp else 0, C=Cc)


def scatter_bwd_launch(L, p, with_gsums):
    keep = Keep()
    out = torch.full((p["T"] + 1, p["ld"]), SENT, device="cuda")
    S = gsums_buf(p["C"]) if with_gsums else None
    d = edge_desc(L, K_SCATTER_BWD, keep, g=p["csr"], bn=p["bn"], a=_cu(p["dM"]), b=None if p["dP"] is None else _cu(p["dP"]), c=_cu(p["A2"]),
                  out=out, gsums=S, ldb=0 if p["dP"] is None else p["dP"].shape[1], col0=p["dpcol0"], ldc=p["ld"], H=p["H"], D=p["D"], rows=p["T"],
                  cstride=p["C"] + 3)
    keep.m.append(d)
    return d, out, S, keep


def scatter_bwd_check(p, out, S, tag):
    out = out.cpu()
    _untouched(out[p["T"]:], tag + ": the row behind T")
    _untouched(out[:, p["C"]:], tag + ": columns behind 2H + D")
    a = (p["dM"], p["dP"], p["dpcol0"], p["A2"], p["H"], p["D"], p["bn"], p["csr"].s, p["csr"].o)
    rg, rs = V.scatter_avg_bwd(*a)
    e, tol = _assert_close(out[:p["T"], :p["C"]], rg, 2e-6, 1e-6, tag + " g2", "64x4 RPT 4")
    line = "%s: g2 err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, _yard(V.scatter_avg_bwd, *a))
    if S is not None:
        line += check_gsums(S, rs, p["C"], tag, "64x4 RPT 4")
    print(line)


@pytest.mark.parametrize("H,D", [(4, 4), (124, 12), (128, 8)])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 32, 33, 130])
def test_scatter_avg_bwd(T, H, D):
    """T around the 16 rows of a pass and the 32 of a workgroup; 130 is a third workgroup with a tail of two rows behind the 64 rows
    per workgroup of the SLN_SCATTER_NIT = 4 form (the lab-switch test below); 2H + D = 260 crosses the 256-column block; dP absent, and at
    column 8 of a wider array; statistics absent and accumulated onto a non-zero start."""
    L = _lib()
    for bnmode in (("eval", "none") if T == 1 else ("train", "eval")):
        for with_dp in (False, True):
            for with_gsums in (False, True):
                p = scatter_bwd_problem(L, T, H, D, bnmode, with_dp)
                d, out, S, keep = scatter_bwd_launch(L, p, with_gsums)
                rc, _ = launch_edge(L, [d], what="scatter_avg_bwd T=%d H=%d" % (T, H))
                assert rc == 0, rc
                scatter_bwd_check(p, out, S, "scatter_bwd[T=%d H=%d D=%d %s dP=%d gs=%d]" % (T, H, D, bnmode, with_dp, with_gsums))


def gather_bwd_problem(L, D, gkey, masked, with_add, seed=0):
    tri, O = GRAPHS[gkey]()
    csr = HostCsr(L, tri, O)
    g = GC._seed("gather-bwd", D, gkey, masked, with_add, seed)
    bn, xprev = None, None
    if masked:
        x, bn = masked_input("eval" if O == 1 else "train", g, GC._randn(g, O, D))
        xprev = torch.cat([x, GC._randn(g, O, 4)], 1).contiguous()
    return dict(csr=csr, D=D, O=O, masked=masked, bn=bn, xprev=xprev, dG=GC._randn(g, csr.T, 3 * D + 4),
                add1=GC._randn(g, O, D + 8) if with_add else None)


def gather_bwd_launch(L, p):
    keep = Keep()
    D = p["D"]
    out = torch.full((p["O"] + 1, D + 4), SENT, device="cuda")
    S = gsums_buf(D) if p["masked"] else None
    d = edge_desc(L, K_GATHER_BWD, keep, g=p["csr"], bn=p["bn"], a=_cu(p["dG"]), b=None if p["add1"] is None else _cu(p["add1"]),
                  c=None if p["xprev"] is None else _cu(p["xprev"]), out=out, gsums=S, lda=3 * D + 4, ldb=D + 8 if p["add1"] is not None else 0,
                  ldc=D + 4 if p["masked"] else 0, ldo=D + 4, D=D, rows=p["O"], cstride=D + 3, masked=p["masked"])
    keep.m.append(d)
    return d, out, S, keep


def gather_bwd_check(p, out, S, tag, form):
    out, D, O = out.cpu(), p["D"], p["O"]
    _untouched(out[O:], tag + ": the row behind O")
    _untouched(out[:, D:], tag + ": columns behind D")
    a = (p["dG"], D, p["csr"].s, p["csr"].o, O, p["add1"], p["xprev"], p["bn"], p["masked"])
    rd, rs = V.gather_bwd(*a)
    e, tol = _assert_close(out[:O, :D], rd, 2e-6, 1e-6, tag + " dX", form)
    line = "%s: dX err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, _yard(V.gather_bwd, *a))
    if S is not None:
        line += check_gsums(S, rs, D, tag, form)
    print(line)


@pytest.mark.parametrize("O", [1, 17])
@pytest.mark.parametrize("D", [4, 64, 68, 132])
def test_gather_bwd(D, O):
    """Both variants (D <= 64: 16 x 16, above: 32 x 16) and a second column block (132 over 128); plain and masked; with and
    without the second gradient, which has its own stride; the degree ladder 0 .. 80 with a sink above 200."""
    L = _lib()
    for masked in (0, 1):
        for with_add in (False, True):
            p = gather_bwd_problem(L, D, O, masked, with_add)
            d, out, S, keep = gather_bwd_launch(L, p)
            rc, _ = launch_edge(L, [d], what="gather_bwd D=%d O=%d" % (D, O))
            assert rc == 0, rc
            gather_bwd_check(p, out, S, "gather_bwd[D=%d O=%d masked=%d add1=%d]" % (D, O, masked, with_add), "32x16" if D > 64 else "16x16")


def mask_gstats_problem(rows, cols, with_d2, seed=0):
    g = GC._seed("mask-gstats", rows, cols, with_d2, seed)
    x, bn = masked_input("eval" if rows == 1 else "train", g, GC._randn(g, rows, cols))
    return dict(rows=rows, cols=cols, bn=bn, xprev=torch.cat([x, GC._randn(g, rows, 2)], 1).contiguous(), d1=GC._randn(g, rows, cols + 1),
                d2=GC._randn(g, rows, cols + 5) if with_d2 else None)


def mask_gstats_launch(L, p):
    keep = Keep()
    rows, cols = p["rows"], p["cols"]
    out = torch.full((rows + 1, cols + 3), SENT, device="cuda")
    S = gsums_buf(cols)
    d = edge_desc(L, K_MASK_GSTATS, keep, bn=p["bn"], a=_cu(p["d1"]), b=None if p["d2"] is None else _cu(p["d2"]), c=_cu(p["xprev"]), out=out,
                  gsums=S, lda=cols + 1, ldb=cols + 5 if p["d2"] is not None else 0, ldc=cols + 2, ldo=cols + 3, rows=rows, cols=cols, cstride=cols + 3)
    keep.m.append(d)
    return d, out, S, keep


def mask_gstats_check(p, out, S, tag):
    out, rows, cols = out.cpu(), p["rows"], p["cols"]
    _untouched(out[rows:], tag + ": the row behind the last")
    _untouched(out[:, cols:], tag + ": columns behind the last")
    a = (p["d1"], p["d2"], p["xprev"], p["bn"], rows, cols)
    rd, rs = V.mask_gstats(*a)
    e, tol = _assert_close(out[:rows, :cols], rd, 2e-6, 1e-6, tag + " g", "64x4 over 32 rows")
    print("%s: g err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, _yard(V.mask_gstats, *a)) + check_gsums(S, rs, cols, tag, "64x4 over 32 rows"))


@pytest.mark.parametrize("cols", [1, 63, 64, 65])
@pytest.mark.parametrize("rows", [1, 31, 32, 33])
def test_mask_gstats(rows, cols):
    L = _lib()
    for with_d2 in (False, True):
        p = mask_gstats_problem(rows, cols, with_d2)
        d, out, S, keep = mask_gstats_launch(L, p)
        rc, _ = launch_edge(L, [d], what="mask_gstats %dx%d" % (rows, cols))
        assert rc == 0, rc
        mask_gstats_check(p, out, S, "mask_gstats[%dx%d d2=%d]" % (rows, cols, with_d2))


@pytest.mark.parametrize("bnmode", ["none", "train", "eval"])
def test_bn_relu_apply_and_add2(bnmode):
    L = _lib()
    g = GC._seed("apply", bnmode)
    rows, cols, col0 = 37, 70, 8
    x = GC._randn(g, rows, col0 + cols + 3)
    bn = make_bn(bnmode, g, x[:, col0:col0 + cols].contiguous())
    keep = Keep()
    out = torch.full((rows + 1, cols + 2), SENT, device="cuda")
    d = edge_desc(L, K_BN_RELU, keep, bn=bn, a=_cu(x), out=out, lda=x.shape[1], ldo=cols + 2, rows=rows, cols=cols, col0=col0)
    rc, _ = launch_edge(L, [d], what="bn_relu_apply")
    assert rc == 0, rc
    o = out.cpu()
    _untouched(o[rows:], "bn_relu_apply: row behind the last"); _untouched(o[:, cols:], "bn_relu_apply: columns behind the last")
    e, tol = _assert_close(o[:rows, :cols], V.bn_relu_apply(x, col0, cols, bn), 2e-6, 1e-6, "bn_relu_apply " + bnmode, "element-wise")
    print("bn_relu_apply[%s]: err %.3e bound %.3e fp32-yardstick %.3e" % (bnmode, e, tol, _yard(V.bn_relu_apply, x, col0, cols, bn)))
    b = GC._randn(g, rows, cols + 5)
    out2 = torch.full((rows + 1, cols + 2), SENT, device="cuda")
    d2 = edge_desc(L, K_ADD2, keep, a=_cu(x), b=_cu(b), out=out2, lda=x.shape[1], ldb=cols + 5, ldo=cols + 2, rows=rows, cols=cols)
    rc, _ = launch_edge(L, [d2], what="add2")
    assert rc == 0, rc
    o2 = out2.cpu()
    _untouched(o2[rows:], "add2: row behind the last"); _untouched(o2[:, cols:], "add2: columns behind the last")
    assert torch.equal(o2[:rows, :cols], x[:, :cols] + b[:, :cols]), "add2 is one fp32 addition per element: exact"


# ================================================================================================= room-table forms
def test_multi_scatter_avg_fwd_is_the_single_room_launch_room_by_room():
    """Three rooms of different O, T and degree ladders that share the 32 x 8 variant in ONE launch: the smaller rooms'
    workgroups leave.  No atomics: bit-identical to each room's own launch.  Rooms of H = 128 and H = 132 take different
    variants: the hook refuses the set (the engine splits such a step) and nothing is written."""
    L = _lib()
    probs = [scatter_fwd_problem(L, 128, 8, "train", k, seed=k) for k in (9, 1, 5)]
    singles = []
    for p in probs:
        d, out, keep = scatter_fwd_launch(L, p)
        assert launch_edge(L, [d], what="scatter_avg_fwd single")[0] == 0
        singles.append(out.cpu())
    built = [scatter_fwd_launch(L, p) for p in probs]
    rc, var = launch_edge(L, [b[0] for b in built], multi=1, what="scatter_avg_fwd_multi")
    assert rc == 0 and var == 1, (rc, var)              # MV_SCATTER_FWD_32x8
    for i, p in enumerate(probs):
        assert torch.equal(built[i][1].cpu(), singles[i]), "room %d differs from its own launch" % i
        scatter_fwd_check(p, built[i][1], "multi scatter_fwd room %d (O=%d T=%d)" % (i, p["O"], p["csr"].T), "multi 32x8")
    mixed = [scatter_fwd_launch(L, scatter_fwd_problem(L, H, 8, "eval", 5)) for H in (128, 132)]
    rc, _ = launch_edge(L, [b[0] for b in mixed], multi=1, what="scatter_avg_fwd_multi mixed")
    assert rc == -2
    for b in mixed:
        _untouched(b[1].cpu(), "output of a refused room set")


def test_multi_scatter_avg_bwd_gather_bwd_and_mask_gstats():
    """Values carry no atomics: bit-identical to the single-room launches.  Column statistics are sums of per-workgroup partials:
    within the 1e-5 bound of the reference (checked) and of the single-room launch."""
    L = _lib()
    # scatter_avg_bwd
    probs = [scatter_bwd_problem(L, T, 124, 12, "train", True, seed=T) for T in (33, 15, 70)]
    for kind, problems, launch, check, var_expected in (
            ("scatter_bwd", probs, lambda p: scatter_bwd_launch(L, p, True), lambda p, b, t: scatter_bwd_check(p, b[1], b[2], t), 0),
            ("gather_bwd", [gather_bwd_problem(L, 68, k, 1, True, seed=k) for k in (17, 1, 9)], lambda p: gather_bwd_launch(L, p),
             lambda p, b, t: gather_bwd_check(p, b[1], b[2], t, "multi 32x16"), 0),
            ("mask_gstats", [mask_gstats_problem(r, c, True, seed=r) for r, c in ((33, 65), (1, 65), (70, 3))], lambda p: mask_gstats_launch(L, p),
             lambda p, b, t: mask_gstats_check(p, b[1], b[2], t), 0)):
        singles = []
        for p in problems:
            b = launch(p)
            assert launch_edge(L, [b[0]], what=kind + " single")[0] == 0
            singles.append((b[1].cpu(), b[2].cpu()))
        built = [launch(p) for p in problems]
        rc, var = launch_edge(L, [b[0] for b in built], multi=1, what=kind + "_multi")
        assert rc == 0 and var == var_expected, (kind, rc, var)
        for i, p in enumerate(problems):
            assert torch.equal(built[i][1].cpu(), singles[i][0]), "%s room %d differs from its own launch" % (kind, i)
            check(p, built[i], "multi %s room %d" % (kind, i))
            Cc = singles[i][1].shape[1] - 3
            for r in range(2):
                _assert_close(built[i][2].cpu()[r, :Cc], singles[i][1][r, :Cc], 1e-5, 1e-5, "multi %s room %d gsums[%d] vs single" % (kind, i, r), kind)
    mixed = [gather_bwd_launch(L, gather_bwd_problem(L, D, 9, 1, False)) for D in (64, 68)]
    rc, _ = launch_edge(L, [b[0] for b in mixed], multi=1, what="gather_bwd_multi mixed")
    assert rc == -2
    for b in mixed:
        _untouched(b[1].cpu(), "output of a refused room set")


def test_multi_add2_is_exact_room_by_room():
    L = _lib()
    rooms = []
    for rows, cols in ((33, 65), (1, 3), (7, 300)):
        g = GC._seed("multi-add2", rows, cols)
        a, b = GC._randn(g, rows, cols + 4), GC._randn(g, rows, cols + 1)
        keep, out = Keep(), torch.full((rows + 1, cols + 2), SENT, device="cuda")
        rooms.append((edge_desc(L, K_ADD2, keep, a=_cu(a), b=_cu(b), out=out, lda=cols + 4, ldb=cols + 1, ldo=cols + 2, rows=rows, cols=cols), out, a, b, keep))
    rc, var = launch_edge(L, [r[0] for r in rooms], multi=1, what="add2_multi")
    assert rc == 0 and var == 0, (rc, var)
    for d, out, a, b, keep in rooms:
        o, (rows, cols) = out.cpu(), (a.shape[0], b.shape[1] - 1)
        _untouched(o[rows:], "add2_multi: row behind the last"); _untouched(o[:, cols:], "add2_multi: columns behind the last")
        assert torch.equal(o[:rows, :cols], a[:, :cols] + b[:, :cols]), "add2_multi is one fp32 addition per element: exact"


# ================================================================================================= CSR build
def run_csr(L, tri, O, num_preds, edges_only=False, deg_is_zero=False):
    T = tri.shape[0]
    i32 = lambda n, fill: torch.full((n,), fill, dtype=torch.int32, device="cuda")
    t = dict(s=i32(T + 1, -7), p=i32(T + 1, -7), o=i32(T + 1, -7), deg=i32(O + 1, 0 if deg_is_zero else 12345), invdeg=torch.full((O + 1,), SENT, device="cuda"),
             rowptr=i32(O + 2, -7), cursor=i32(O + 1, -7), ent=i32(2 * T + 1, -7))
    if deg_is_zero:
        t["deg"][O] = -7
    err = torch.zeros(2, dtype=torch.int32, device="cuda"); err[1] = -7
    d = csr_desc(L, t, T, O)
    src = _cu(tri[:, [0, 2]] if edges_only else tri)
    rc = L.lib().sln_debug_vae_csr(_p(src) if T else None, num_preds, int(edges_only), int(deg_is_zero), C.byref(d), _p(err), L.current_stream_ptr())
    _sync("sln_debug_vae_csr T=%d O=%d" % (T, O))
    assert rc == 0, rc
    return {k: v.cpu() for k, v in t.items()}, err.cpu()


def check_csr(got, err, tri, O, num_preds, edges_only, tag):
    T = tri.shape[0]
    ref = V.csr(tri[:, [0, 2]] if edges_only else tri, O, num_preds, edges_only)
    assert int(err[0]) == ref["err"] and int(err[1]) == -7, tag
    for k in ("s", "p", "o"):
        assert torch.equal(got[k][:T], ref[k]) and int(got[k][T]) == -7, "%s: %s" % (tag, k)
    assert torch.equal(got["deg"][:O], ref["deg"]), tag
    assert int(got["deg"][O]) in (-7, 12345) and int(got["rowptr"][O + 1]) == -7 and int(got["cursor"][O]) == -7 and int(got["ent"][2 * T]) == -7, tag
    assert float(got["invdeg"][O]) == SENT
    rp = torch.zeros(O + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(got["deg"][:O].long(), 0)
    assert torch.equal(got["rowptr"][:O + 1].long(), rp), tag + ": rowptr is not the exclusive scan of deg"
    want = 1.0 / ref["deg"].clamp_min(1).float()
    ulp = (got["invdeg"][:O].view(torch.int32) - want.view(torch.int32)).abs().max()
    assert int(ulp) <= 1, "%s: invdeg %d ulp from 1 / max(deg, 1)" % (tag, int(ulp))
    ent = got["ent"][:2 * T].tolist()
    for i in range(O):
        row = ent[int(rp[i]):int(rp[i + 1])]
        assert all(a < b for a, b in zip(row, row[1:])), "%s: row %d is not strictly ascending" % (tag, i)
        assert row == ref["rows"][i], "%s: row %d holds other entries" % (tag, i)
    assert sorted(ent) == list(range(2 * T)), tag


def test_csr_build():
    """A self-loop in a one-row graph; no triples; the scan's carry over its 1 024 chunk; ONE graph with rows of degree 0, 1, 2, 64, 65, 1 024 and
    1 025 (the last and the sink take the serial sort of one lane beside rows sorted in LDS); the edges-only form; both values of deg_is_zero."""
    L = _lib()
    g = GC._seed("csr")
    big, bigO = ladder_graph([0, 1, 2, 64, 65, 1024, 1025], 1)        # one launch sorts rows in LDS and serially; the sink gets 1 093
    cases = {"self-loop": (loops_graph(1)[0], 1), "empty": (torch.zeros(0, 3, dtype=torch.int64), 5),
             "carry": (torch.stack([torch.randint(0, 1030, (1500,), generator=g), torch.randint(0, 4, (1500,), generator=g),
                                    torch.randint(0, 1030, (1500,), generator=g)], 1), 1030),
             "ladder": (big, bigO)}
    for name, (tri, O) in cases.items():
        for edges_only in (False, True):
            for dz in (False, True):
                got, err = run_csr(L, tri, O, 5, edges_only, dz)
                check_csr(got, err, tri, O, 5, edges_only, "csr[%s edges=%d deg_is_zero=%d]" % (name, edges_only, dz))
    assert V.csr(big, bigO, 5)["deg"].tolist() == [0, 1, 2, 64, 65, 1024, 1025, 1093]


@pytest.mark.parametrize("col,val", [(0, 7), (0, -1), (1, 5), (1, -2), (2, 7)])
def test_csr_flags_and_neutralises_an_out_of_range_id(col, val):
    L = _lib()
    tri, O = ladder_graph([2, 3, 1], 3)
    tri[2, col] = val
    got, err = run_csr(L, tri, O, 5)
    assert int(err[0]) == 1 and (int(got["s"][2]), int(got["p"][2]), int(got["o"][2])) == (0, 0, 0)
    check_csr(got, err, tri, O, 5, False, "csr[bad column %d = %d]" % (col, val))


# ================================================================================================= loss
def loss_desc(L, **kw):
    d = L.SlnDbgLoss()
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, _p(v) if isinstance(v, torch.Tensor) or v is None else v)
    return d


LOSS_FORMS = [(1, 1, 0, 0), (1, 0, 1, 1), (0, 1, 1, 0), (0, 0, 0, 1), (1, 1, 0, 1)]      # (from_logits, grads, use_ae, acc_prezeroed)


@pytest.mark.parametrize("n_angle", [1, 7, 8, 9, 24])
@pytest.mark.parametrize("O", [1, 7, 33, 2049])
def test_loss(O, n_angle):
    """O = 2 049: the second trip of the row loop (2 048 rows per trip) and, with n_z = 32, KL elements behind 4 x stride.
    n_angle around the eight lanes of a row.  One row holds logits of +80 and -80; targets sit on the first and the last bin."""
    L = _lib()
    g = GC._seed("loss", O, n_angle)
    bd, nz, w = 6, 32 if O == 2049 else 8, 0.37
    boxes, bp = torch.rand(O, bd, generator=g), torch.rand(O, bd, generator=g)
    logits = 3 * GC._randn(g, O, n_angle)
    logits[0, 0] = 80.0
    if n_angle > 1:
        logits[0, 1] = -80.0
    angles = torch.randint(0, n_angle, (O,), generator=g)
    angles[0], angles[O - 1] = 0, n_angle - 1
    mu, lv = GC._randn(g, O, nz), 0.5 * GC._randn(g, O, nz)
    klw = torch.tensor([w])
    lp_in = V.log_softmax(logits).float()
    for fl, grads, ae, pz in LOSS_FORMS:
        tag = "loss[O=%d n=%d from_logits=%d grads=%d ae=%d prezeroed=%d]" % (O, n_angle, fl, grads, ae, pz)
        ap = torch.full((O + 1, n_angle), SENT, device="cuda")
        if not fl:
            ap[:O] = lp_in.cuda()
        acc = torch.zeros(5, dtype=F64, device="cuda") if pz else torch.full((5,), SENT, dtype=F64, device="cuda")
        acc[4] = SENT
        losses = torch.full((5,), SENT, device="cuda")
        dbp = torch.full((O + 1, 8), SENT, device="cuda") if grads else None
        dlg = torch.full((O + 1, n_angle), SENT, device="cuda") if grads else None
        keep = [_cu(boxes), _cu(bp), _cu(angles), _cu(logits), _cu(mu), _cu(lv), _cu(klw)]
        d = loss_desc(L, kind=0, boxes=keep[0], boxes_pred=keep[1], angles=keep[2], logits=keep[3] if fl else None, angles_pred=ap, mu=keep[4],
                      logvar=keep[5], kl_weight=keep[6], acc=acc, losses=losses, d_boxes_pred=dbp, d_logits=dlg, O=O, box_dim=bd, n_angle=n_angle,
                      n_z=nz, use_ae=ae, ld_dbp=8, acc_prezeroed=pz, from_logits=fl)
        rc = L.lib().sln_debug_vae_loss(C.byref(d), L.current_stream_ptr())
        _sync(tag)
        assert rc == 0, rc
        a = (boxes, bp, angles, logits if fl else None, None if fl else lp_in, mu, lv, w, ae, fl)
        ref, y32 = V.loss(*a), V.loss(*a, dtype=F32)
        got_l, apc = losses.cpu(), ap.cpu()
        assert float(got_l[4]) == SENT and float(acc.cpu()[4]) == SENT, tag
        line = tag + ":"
        for i, name in enumerate(("bbox", "angle", "kl", "total")):
            e, tol = _assert_close(got_l[i:i + 1], ref["losses"][i:i + 1], 2e-6, 1e-6, "%s %s" % (tag, name), "loss_kernel")
            line += " %s err %.3e bound %.3e fp32-yardstick %.3e |" % (name, e, tol, abs(float(y32["losses"][i]) - float(ref["losses"][i])))
        if ae:
            assert float(got_l[2]) == 0.0, tag
        _untouched(apc[O:], tag + ": angles_pred behind row O")
        if fl:
            e, tol = _assert_close(apc[:O], ref["angles_pred"], 2e-6, 1e-6, tag + " angles_pred", "loss_kernel")
            line += " angles_pred err %.3e bound %.3e fp32-yardstick %.3e |" % (e, tol, float((y32["angles_pred"].double() - ref["angles_pred"]).abs().max()))
        else:
            assert torch.equal(apc[:O], lp_in), tag + ": angles_pred is an input here"
        if grads:
            dbc, dlc = dbp.cpu(), dlg.cpu()
            _untouched(dbc[O:], tag + ": d_boxes_pred behind row O"); _untouched(dbc[:, bd:], tag + ": ld_dbp padding")
            _untouched(dlc[O:], tag + ": d_logits behind row O")
            e1, t1 = _assert_close(dbc[:O, :bd], ref["d_boxes_pred"], 2e-6, 1e-6, tag + " d_boxes_pred", "loss_kernel")
            e2, t2 = _assert_close(dlc[:O], ref["d_logits"], 2e-6, 1e-6, tag + " d_logits", "loss_kernel")
            line += " d_boxes_pred err %.3e bound %.3e | d_logits err %.3e bound %.3e fp32-yardstick %.3e" % (
                e1, t1, e2, t2, float((y32["d_logits"].double() - ref["d_logits"]).abs().max()))
        print(line)


@pytest.mark.parametrize("O", [1, 129])
def test_latent_bwd_log_softmax_and_its_backward(O):
    L = _lib()
    g = GC._seed("latent", O)
    nz, n, w = 8, 24, 0.37
    mu, lv, eps, dz = GC._randn(g, O, nz), 0.5 * GC._randn(g, O, nz), GC._randn(g, O, nz), GC._randn(g, O, nz)
    klw = _cu(torch.tensor([w]))
    for ae in (0, 1):
        dmu, dlv = torch.full((O + 1, nz), SENT, device="cuda"), torch.full((O + 1, nz), SENT, device="cuda")
        keep = [_cu(mu), _cu(lv), _cu(eps), _cu(dz)]
        d = loss_desc(L, kind=3, mu=keep[0], logvar=keep[1], eps=keep[2], dz=keep[3], kl_weight=klw, dmu=dmu, dlogvar=dlv, O=O, n_z=nz, use_ae=ae)
        rc = L.lib().sln_debug_vae_loss(C.byref(d), L.current_stream_ptr())
        _sync("latent_bwd")
        assert rc == 0, rc
        rm, rl = V.latent_bwd(mu, lv, eps, dz, w, ae)
        _untouched(dmu.cpu()[O:], "dmu behind row O"); _untouched(dlv.cpu()[O:], "dlogvar behind row O")
        e1, t1 = _assert_close(dmu.cpu()[:O], rm, 2e-6, 1e-6, "latent_bwd dmu", "latent_bwd")
        e2, t2 = _assert_close(dlv.cpu()[:O], rl, 2e-6, 1e-6, "latent_bwd dlogvar", "latent_bwd")
        print("latent_bwd[O=%d ae=%d]: dmu err %.3e bound %.3e dlogvar err %.3e bound %.3e fp32-yardstick %.3e" % (
            O, ae, e1, t1, e2, t2, _yard(V.latent_bwd, mu, lv, eps, dz, w, ae)))
    x = 3 * GC._randn(g, O, n)
    x[0, 0], x[0, 1] = 80.0, -80.0
    y = torch.full((O + 1, n), SENT, device="cuda")
    xd = _cu(x)
    rc = L.lib().sln_debug_vae_loss(C.byref(loss_desc(L, kind=1, logits=xd, angles_pred=y, O=O, n_angle=n)), L.current_stream_ptr())
    _sync("log_softmax")
    assert rc == 0, rc
    _untouched(y.cpu()[O:], "log_softmax behind row O")
    e, tol = _assert_close(y.cpu()[:O], V.log_softmax(x), 2e-6, 1e-6, "log_softmax", "row per thread")
    print("log_softmax[O=%d]: err %.3e bound %.3e fp32-yardstick %.3e" % (O, e, tol, _yard(V.log_softmax, x)))
    lp, dlp = V.log_softmax(x).float(), GC._randn(g, O, n)
    dx = torch.full((O + 1, n), SENT, device="cuda")
    lpd, dlpd = _cu(lp), _cu(dlp)
    rc = L.lib().sln_debug_vae_loss(C.byref(loss_desc(L, kind=2, angles_pred=lpd, d_logprob=dlpd, d_logits=dx, O=O, n_angle=n)), L.current_stream_ptr())
    _sync("log_softmax_bwd")
    assert rc == 0, rc
    _untouched(dx.cpu()[O:], "log_softmax_bwd behind row O")
    e, tol = _assert_close(dx.cpu()[:O], V.log_softmax_bwd(lp, dlp), 2e-6, 1e-6, "log_softmax_bwd", "row per thread")
    print("log_softmax_bwd[O=%d]: err %.3e bound %.3e fp32-yardstick %.3e" % (O, e, tol, _yard(V.log_softmax_bwd, lp, dlp)))


# ================================================================================================= BatchNorm tables, transposes
def bn_table_entries(g):
    """-> list of dict(C, rows, sums [2, C + 3] fp64, gsums, with_running): C 1 / 256 / 257, the batch's triple count, its
    object count (1: no Bessel factor), an explicit count; column 0 of the second entry has E[x^2] - mean^2 slightly negative"""
    out = []
    for C_, rows, n_eff in ((1, -1, 7), (256, -2, 1), (257, 12, 12), (5, 12, 12)):
        x = 2.0 * GC._randn(g, n_eff, C_) + 1.0
        sums = torch.cat([V.sums_of(x), torch.full((2, 3), 1e30, dtype=F64)], 1).contiguous()
        if C_ == 257:
            sums[0, 0], sums[1, 0] = 12 * 3.0, 12 * 9.0 * (1 - 1e-12)
        gs = torch.cat([GC._randn(g, 2, C_).double(), torch.full((2, 3), 1e30, dtype=F64)], 1).contiguous()
        out.append(dict(C=C_, rows=rows, n_eff=n_eff, sums=sums, gsums=gs, running=C_ != 5))
    return out


def run_bn_table(L, kind, entries, bufs, independent, mom=0.1, rows_t=7, rows_o=1):
    arr = (L.SlnDbgBnEntry * len(entries))()
    keep = []
    for i, (e, b) in enumerate(zip(entries, bufs)):
        sd, gd = _cu(e["sums"]), _cu(e["gsums"])
        keep += [sd, gd]
        arr[i].sums, arr[i].gsums, arr[i].cstride, arr[i].C, arr[i].rows = _p(sd), _p(gd), e["C"] + 3, e["C"], e["rows"]
        for k in ("rmean", "rvar", "nbt", "dgamma", "dbeta"):
            setattr(arr[i], k, _p(b.get(k)))
    rc = L.lib().sln_debug_vae_tables(kind, arr, len(entries), max(e["C"] for e in entries), mom, independent, rows_t, rows_o, L.current_stream_ptr())
    _sync("sln_debug_vae_tables kind %d" % kind)
    assert rc == 0, rc


def test_bn_running_update_and_param_grads():
    L = _lib()
    g = GC._seed("bn-tables")
    entries = bn_table_entries(g)
    bufs, start = [], []
    for e in entries:
        C_ = e["C"]
        rm0, rv0 = 0.3 * GC._randn(g, C_), GC._uniform(g, C_, 0.5, 2.0)
        dg0, db0 = GC._randn(g, C_), GC._randn(g, C_)
        pad = lambda t: _cu(torch.cat([t, torch.full((2,), SENT)]))
        b = dict(nbt=torch.tensor([5, -7], dtype=torch.int64, device="cuda"), dgamma=pad(dg0), dbeta=pad(db0))
        if e["running"]:
            b.update(rmean=pad(rm0), rvar=pad(rv0))
        bufs.append(b); start.append((rm0, rv0, dg0, db0))
    run_bn_table(L, 0, entries, bufs, 1)
    run_bn_table(L, 1, entries, bufs, 1)
    for e, b, (rm0, rv0, dg0, db0) in zip(entries, bufs, start):
        C_, tag = e["C"], "bn table entry C=%d rows=%d" % (e["C"], e["rows"])
        assert b["nbt"].cpu().tolist() == [6, -7], tag
        if e["running"]:
            a = (e["sums"], C_, e["n_eff"], rm0, rv0, 0.1)
            rm, rv = V.bn_running_update(*a)
            gm, gv = b["rmean"].cpu(), b["rvar"].cpu()
            _untouched(gm[C_:], tag + ": rmean behind C"); _untouched(gv[C_:], tag + ": rvar behind C")
            e1, t1 = _assert_close(gm[:C_], rm, 2e-6, 1e-6, tag + " rmean", "one thread per column")
            e2, t2 = _assert_close(gv[:C_], rv, 2e-6, 1e-6, tag + " rvar", "one thread per column")
            print("%s: rmean err %.3e bound %.3e rvar err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e1, t1, e2, t2, _yard(V.bn_running_update, *a)))
            if C_ == 257:
                assert abs(float(gv[0]) - 0.9 * float(rv0[0])) <= 1e-6, "a negative variance is clamped to zero"
        rg, rb = V.bn_param_grads(e["gsums"], C_, dg0, db0)
        gg, gb = b["dgamma"].cpu(), b["dbeta"].cpu()
        _untouched(gg[C_:], tag + ": dgamma behind C"); _untouched(gb[C_:], tag + ": dbeta behind C")
        e1, t1 = _assert_close(gg[:C_], rg, 1e-5, 1e-5, tag + " dgamma", "one thread per column")
        e2, t2 = _assert_close(gb[:C_], rb, 1e-5, 1e-5, tag + " dbeta", "one thread per column")
        print("%s: dgamma err %.3e bound %.3e dbeta err %.3e bound %.3e" % (tag, e1, t1, e2, t2))


def test_bn_tables_of_a_shared_module_update_in_order():
    """independent = 0, one module listed twice (recurrent mode): two ordered updates of the same buffers, nbt += 2, both
    applications' gradients added."""
    L = _lib()
    g = GC._seed("bn-shared")
    C_ = 70
    entries = []
    for k in range(2):
        x = (k + 1.0) * GC._randn(g, 9, C_) + k
        entries.append(dict(C=C_, rows=9, n_eff=9, sums=torch.cat([V.sums_of(x), torch.full((2, 3), 1e30, dtype=F64)], 1).contiguous(),
                            gsums=torch.cat([GC._randn(g, 2, C_).double(), torch.full((2, 3), 1e30, dtype=F64)], 1).contiguous()))
    rm0, rv0, dg0, db0 = 0.3 * GC._randn(g, C_), GC._uniform(g, C_, 0.5, 2.0), GC._randn(g, C_), GC._randn(g, C_)
    b = dict(rmean=_cu(rm0), rvar=_cu(rv0), nbt=torch.tensor([0], dtype=torch.int64, device="cuda"), dgamma=_cu(dg0), dbeta=_cu(db0))
    run_bn_table(L, 0, entries, [b, b], 0)
    run_bn_table(L, 1, entries, [b, b], 0)
    rm, rv, dg, db = rm0.double(), rv0.double(), dg0.double(), db0.double()
    for e in entries:
        rm, rv = V.bn_running_update(e["sums"], C_, 9, rm, rv, 0.1)
        dg, db = V.bn_param_grads(e["gsums"], C_, dg, db)
    assert int(b["nbt"].cpu()[0]) == 2
    for name, got, ref, tol in (("rmean", b["rmean"], rm, 2e-6), ("rvar", b["rvar"], rv, 2e-6), ("dgamma", b["dgamma"], dg, 1e-5), ("dbeta", b["dbeta"], db, 1e-5)):
        e_, t_ = _assert_close(got.cpu(), ref, tol, tol / 2 if tol == 2e-6 else tol, "shared module " + name, "sequential entries")
        print("shared module %s: err %.3e bound %.3e" % (name, e_, t_))


def test_transpose_table():
    """Five entries in one launch, max_tiles (6) above the small entries' tile counts, dst_ld > rows: exact, padding untouched"""
    L = _lib()
    g = GC._seed("transpose")
    shapes = [(1, 1), (31, 33), (32, 32), (33, 65), (100, 7)]
    arr = (L.SlnDbgTranspose * len(shapes))()
    src, dst = [], []
    for i, (r, c) in enumerate(shapes):
        src.append(GC._randn(g, r, c)); dst.append(torch.full((c + 1, r + 3), SENT, device="cuda"))
        sd = _cu(src[-1]); src.append(sd)
        arr[i].src, arr[i].dst, arr[i].rows, arr[i].cols, arr[i].dst_ld = _p(sd), _p(dst[-1]), r, c, r + 3
    rc = L.lib().sln_debug_vae_tables(2, arr, len(shapes), 6, 0.0, 0, 0, 0, L.current_stream_ptr())
    _sync("transpose_table")
    assert rc == 0, rc
    for i, (r, c) in enumerate(shapes):
        o = dst[i].cpu()
        assert torch.equal(o[:c, :r], src[2 * i].t()), "transpose %dx%d" % (r, c)
        _untouched(o[c:], "transpose %dx%d: row behind the last" % (r, c)); _untouched(o[:, r:], "transpose %dx%d: dst_ld padding" % (r, c))


# ================================================================================================= Adam, the Philox draw
def run_opt(L, **kw):
    d = L.SlnDbgOpt()
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, _p(v) if isinstance(v, torch.Tensor) or v is None else v)
    rc = L.lib().sln_debug_vae_opt(C.byref(d), L.current_stream_ptr())
    _sync("sln_debug_vae_opt kind %d n %d" % (d.kind, d.n))
    assert rc == 0, rc
    return d


ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4096, 4097, 1048581])
def test_adam(n, off):
    """n around the 16-byte vector and the 4 096 elements of a workgroup; 1 048 581 is more than 256 workgroups' worth: the
    grid-stride loop.  Views 4 bytes off alignment take the scalar loop throughout.  A non-finite total loss changes nothing,
    keeps the step and reports skip; two launches in a row find the arrival ticket reset."""
    L = _lib()
    g = GC._seed("adam", n, off)
    p0, grad, m0, v0 = GC._randn(g, n), GC._randn(g, n), 0.1 * GC._randn(g, n), 0.01 * torch.rand(n, generator=g)
    for step, tl, calls in [(0, None, 1), (0, 0.5, 1), (999, 0.5, 1), (999, float("nan"), 1), (0, float("inf"), 1), (0, None, 2)]:
        tag = "adam[n=%d off=%d step=%d loss=%s calls=%d]" % (n, off, step, tl, calls)
        bufs = []
        for t in (p0, grad, m0, v0):
            b = torch.full((n + off + 1,), SENT, device="cuda")
            b[off:off + n] = t.cuda()
            bufs.append(b)
        views = [b[off:off + n] for b in bufs]
        assert all(v.data_ptr() % 16 == 4 * off for v in views)
        tld = None if tl is None else _cu(torch.tensor([tl]))
        d = run_opt(L, kind=0, params=views[0], grads=views[1], m=views[2], v=views[3], total_loss=tld, n=n, step=step, calls=calls, **ADAM)
        got = [b.cpu() for b in bufs]
        for b, name in zip(got, "pgmv"):
            _untouched(b[off + n:], "%s: %s behind n" % (tag, name)); _untouched(b[:off], "%s: %s in front of the view" % (tag, name))
        assert torch.equal(got[1][off:off + n], grad), tag + ": the gradient is an input"
        if tl is not None and not np.isfinite(tl):
            assert d.out_skip == 1 and d.out_step == step, (tag, d.out_skip, d.out_step)
            for b, t, name in zip(got, (p0, grad, m0, v0), "pgmv"):
                assert torch.equal(b[off:off + n], t), "%s: %s changed on a skipped step" % (tag, name)
            continue
        a = (p0, grad, m0, v0, step) + tuple(ADAM[k] for k in ("lr", "beta1", "beta2", "eps"))
        rp, rm, rv, bc1, bc2 = V.adam(*a, calls=calls)
        assert d.out_skip == 0 and d.out_step == step + calls, (tag, d.out_skip, d.out_step)
        assert abs(d.out_bc1 - bc1) <= 2e-6 * bc1 and abs(d.out_bc2 - bc2) <= 2e-6 * bc2, (tag, d.out_bc1, bc1, d.out_bc2, bc2)
        y = V.adam(*a, calls=calls, dtype=F32)
        line = tag + ":"
        for b, ref, y32, name in zip((got[0], got[2], got[3]), (rp, rm, rv), y[:3], ("p", "m", "v")):
            e, tol = _assert_close(b[off:off + n], ref, 2e-6, 1e-6, "%s %s" % (tag, name), "vec" if not off else "scalar")
            line += " %s err %.3e bound %.3e fp32-yardstick %.3e |" % (name, e, tol, float((y32.double() - ref).abs().max()))
        print(line)


RANDN_NS = (1, 3, 4, 5, 1024, 1025)
RANDN_SEED, RANDN_OFFSET = 0xDEADBEEF00000007, (1 << 32) + 3


def randn_bound():
    """four times the largest distance of a float32 numpy evaluation of the draw from the fp64 one, over the counters below"""
    worst = 0.0
    for n in RANDN_NS:
        for k in range(2):
            worst = max(worst, float(np.abs(V.randn(n, RANDN_SEED, RANDN_OFFSET + k, np.float32).astype(np.float64) - V.randn(n, RANDN_SEED, RANDN_OFFSET + k)).max()))
    return worst, 4.0 * worst


@pytest.mark.parametrize("n", RANDN_NS)
def test_randn(n):
    """Values against the numpy Philox (uniforms and the angle in float32 as the kernel forms them, log / sqrt / cos / sin in
    fp64); a seed with its high word set and an offset >= 2^32; the offset advances by exactly one per launch.  The bound is not
    one of the project's: the device's logf / sincosf sit a few ulp from numpy's, so it is FOUR TIMES the largest error of a
    float32 numpy evaluation of the same formulas against the fp64 one over these counters - measured on the CPU: 2.95e-07,
    bound 1.18e-06."""
    L = _lib()
    worst, bound = randn_bound()
    for calls in (1, 2):
        buf = torch.full((n + 1,), SENT, device="cuda")
        d = run_opt(L, kind=1, params=buf, n=n, seed=RANDN_SEED, offset=RANDN_OFFSET, calls=calls)
        assert d.out_offset == RANDN_OFFSET + calls, (d.out_offset, calls)
        got = buf.cpu().numpy().astype(np.float64)
        assert got[n] == SENT, "randn wrote behind n"
        e = float(np.abs(got[:n] - V.randn(n, RANDN_SEED, RANDN_OFFSET + calls - 1)).max())
        print("randn[n=%d launch %d]: err %.3e bound %.3e fp32-yardstick %.3e" % (n, calls, e, bound, worst))
        assert e <= bound, "randn n=%d: max err %.3e > %.3e" % (n, e, bound)


# ================================================================================================= embeddings
M_ENC, M_ENC_BWD, M_DEC, M_DEC_BWD, M_GATHER, M_BWD_I32, M_BWD_I64, M_I64_I32, M_STAGE, M_VALIDATE = range(10)
N_OBJ, N_ATTR, N_ANGLE, N_Z = 8, 5, 6, 12
ASM_OS = [1, 16, 17, 63, 64, 65, 130, 8200]           # 16 / 64 rows per workgroup; 8 200 is past the 8 192 switch to 64
# table rows (obj, attr, angle) -> the route the launcher takes; "big": 1 300 * 8 floats alone pass the 10 240 of the LDS form
ASM_ROUTES = {"lds": (7, 5, 9), "plain-rows0": (0, 0, 0), "plain-big": (1300, 5, 9), "det": (7, 5, 9)}


def embed_desc(L, keep, **kw):
    d = L.SlnDbgEmbed()
    for k, v in kw.items():
        assert hasattr(d, k), k
        if isinstance(v, torch.Tensor) or v is None:
            keep.append(v)
            v = _p(v)
        setattr(d, k, v)
    return d


def launch_embed(L, descs, multi=0, what="embed"):
    arr = (L.SlnDbgEmbed * len(descs))(*descs)
    var = C.c_int(-9)
    rc = L.lib().sln_debug_vae_embed(arr, len(descs), multi, C.byref(var), L.current_stream_ptr())
    _sync("sln_debug_vae_embed " + what)
    return rc, var.value


class deterministic:
    """sln_set_deterministic is process-wide: whatever it was comes back"""

    def __init__(self, L, on):
        self.L, self.on = L, on

    def __enter__(self):
        self.was = self.L.lib().sln_get_deterministic()
        if self.on:
            self.L.lib().sln_set_deterministic(1)

    def __exit__(self, *a):
        self.L.lib().sln_set_deterministic(self.was)


def sent_rows(t, extra=1):
    """a device copy of t with `extra` rows of SENT behind it"""
    out = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), SENT, dtype=t.dtype, device="cuda")
    out[:t.shape[0]] = t.cuda()
    return out


def ids(g, O, rows):
    """ids that leave the LAST table row unnamed (its gradient must stay what it was)"""
    return torch.randint(0, max(rows - 1, 1), (O,), generator=g)


def enc_problem(O, n_attr, n_box, box_dim, rows=(7, 5, 9), seed=0):
    g = GC._seed("enc", O, n_attr, n_box, box_dim, seed)
    ro, ra, rg = (r if r > 0 else v for r, v in zip(rows, (7, 5, 9)))         # rows 0 is an ARGUMENT (plain atomics): the tables keep their size
    p = dict(O=O, n_attr=n_attr, n_box=n_box, box_dim=box_dim, W=N_OBJ + n_attr + n_box + N_ANGLE, rows=rows,
             objs=ids(g, O, ro), attrs=ids(g, O, ra), angles=ids(g, O, rg), boxes=torch.rand(O, box_dim, generator=g),
             obj_emb=GC._randn(g, ro, N_OBJ), attr_emb=GC._randn(g, ra, n_attr) if n_attr else None, angle_emb=GC._randn(g, rg, N_ANGLE),
             wb=GC._randn(g, n_box, box_dim), bb=GC._randn(g, n_box))
    p["dx0"] = GC._randn(g, O, p["W"])
    return p


def enc_ints(p):
    return dict(O=p["O"], n_obj=N_OBJ, n_attr=p["n_attr"], n_box=p["n_box"], n_angle=N_ANGLE, box_dim=p["box_dim"])


def enc_fwd_desc(L, p, keep, x0):
    return embed_desc(L, keep, kind=M_ENC, objs=_cu(p["objs"]), attrs=_cu(p["attrs"]), angles=_cu(p["angles"]), boxes=_cu(p["boxes"]),
                      obj_emb=_cu(p["obj_emb"]), attr_emb=None if p["attr_emb"] is None else _cu(p["attr_emb"]), angle_emb=_cu(p["angle_emb"]),
                      wb=_cu(p["wb"]), bb=_cu(p["bb"]), x0=x0, **enc_ints(p))


@pytest.mark.parametrize("box_dim", [4, 6])
@pytest.mark.parametrize("n_attr", [0, N_ATTR])
def test_enc_assemble(n_attr, box_dim):
    """The three gathers are copies: exact.  The box Linear is box_dim fused multiply-adds: the value bound."""
    L = _lib()
    for O in (1, 65):
        for n_box in (1, 64, 65):
            p = enc_problem(O, n_attr, n_box, box_dim)
            keep, x0 = [], torch.full((O + 1, p["W"]), SENT, device="cuda")
            rc, _ = launch_embed(L, [enc_fwd_desc(L, p, keep, x0)], what="enc_assemble")
            assert rc == 0, rc
            tag = "enc_assemble[O=%d n_attr=%d n_box=%d box_dim=%d]" % (O, n_attr, n_box, box_dim)
            got = x0.cpu()
            _untouched(got[O:], tag + ": the row behind O")
            a = (p["objs"], p["attrs"], p["angles"], p["boxes"], p["obj_emb"], p["attr_emb"], p["angle_emb"], p["wb"], p["bb"])
            ref = V.enc_assemble(*a)
            b0 = N_OBJ + n_attr
            for lo, hi in ((0, b0), (b0 + n_box, p["W"])):
                assert torch.equal(got[:O, lo:hi], ref[:, lo:hi].float()), tag + ": a gathered column differs"
            e, tol = _assert_close(got[:O, b0:b0 + n_box], ref[:, b0:b0 + n_box], 2e-6, 1e-6, tag + " box columns", "enc_assemble")
            print("%s: box err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, _yard(V.enc_assemble, *a)))


def asm_tables(p, names):
    """(prefill on the CPU, device buffer with a SENT row behind) per table: `+=` outputs start from non-zero values"""
    g = GC._seed("asm-tables", p["O"], *names)
    out = {}
    for n in names:
        t0 = GC._randn(g, *p[n].shape)
        out[n] = (t0, sent_rows(t0))
    return out


def check_table(buf, t0, idx, d, col0, n, tag, form):
    got = buf.cpu()
    _untouched(got[t0.shape[0]:], tag + ": the row behind the table")
    ref = V.embed_bwd(idx, d, col0, n, t0)
    named = torch.zeros(t0.shape[0], dtype=torch.bool)
    named[idx] = True
    assert not bool(named[-1]) or t0.shape[0] == 1
    assert torch.equal(got[:t0.shape[0]][~named], t0[~named]), tag + ": a table row no index names changed"
    e, tol = _assert_close(got[:t0.shape[0]], ref, 1e-5, 1e-5, tag, form)
    y = float((V.embed_bwd(idx, d, col0, n, t0, dtype=F32).double() - ref).abs().max())
    return "%s err %.3e bound %.3e fp32-yardstick %.3e" % (tag, e, tol, y)


@pytest.mark.parametrize("route", list(ASM_ROUTES))
@pytest.mark.parametrize("O", ASM_OS)
def test_enc_assemble_bwd(O, route):
    """The three tables and the box Linear's gradient are `+=`: prefill plus sum, at the bound of accumulated tables.  LDS tables,
    plain atomics (rows_* = 0, and tables above 10 240 floats) and the deterministic route, which two runs must repeat bit for bit."""
    L = _lib()
    for n_box, n_attr, box_dim in ((1, N_ATTR, 4), (64, 0, 6), (65, N_ATTR, 6)):
        p = enc_problem(O, n_attr, n_box, box_dim, ASM_ROUTES[route])
        runs = []
        with deterministic(L, route == "det"):
            for _ in range(2 if route == "det" else 1):
                keep = []
                names = ["obj_emb", "angle_emb", "wb", "bb"] + (["attr_emb"] if n_attr else [])
                tabs = asm_tables(p, names)
                dev = {k: v[1] for k, v in tabs.items()}
                d = embed_desc(L, keep, kind=M_ENC_BWD, objs=_cu(p["objs"]), attrs=_cu(p["attrs"]), angles=_cu(p["angles"]), boxes=_cu(p["boxes"]),
                               dx0=_cu(p["dx0"]), d_obj_emb=dev["obj_emb"], d_attr_emb=dev.get("attr_emb"), d_angle_emb=dev["angle_emb"], d_wb=dev["wb"],
                               d_bb=dev["bb"], rows_obj=p["rows"][0], rows_attr=p["rows"][1], rows_angle=p["rows"][2], **enc_ints(p))
                rc, _ = launch_embed(L, [d], what="enc_assemble_bwd " + route)
                assert rc == 0, rc
                runs.append({k: v.cpu() for k, v in dev.items()})
        tag = "enc_assemble_bwd[O=%d %s n_box=%d n_attr=%d]" % (O, route, n_box, n_attr)
        if route == "det":
            assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), tag + ": two deterministic runs differ"
        line = check_table(dev["obj_emb"], tabs["obj_emb"][0], p["objs"], p["dx0"], 0, N_OBJ, tag + " obj", route)
        if n_attr:
            line += " | " + check_table(dev["attr_emb"], tabs["attr_emb"][0], p["attrs"], p["dx0"], N_OBJ, n_attr, tag + " attr", route)
        b0 = N_OBJ + n_attr
        line += " | " + check_table(dev["angle_emb"], tabs["angle_emb"][0], p["angles"], p["dx0"], b0 + n_box, N_ANGLE, tag + " angle", route)
        rw, rb = V.box_linear_bwd(p["dx0"][:, b0:b0 + n_box], p["boxes"], tabs["wb"][0], tabs["bb"][0])
        gw, gb = dev["wb"].cpu(), dev["bb"].cpu()
        _untouched(gw[n_box:], tag + ": d_wb behind n_box"); _untouched(gb[n_box:], tag + ": d_bb behind n_box")
        ew, tw = _assert_close(gw[:n_box], rw, 1e-5, 1e-5, tag + " d_wb", route)
        eb, tb = _assert_close(gb[:n_box], rb, 1e-5, 1e-5, tag + " d_bb", route)
        y32 = V.box_linear_bwd(p["dx0"][:, b0:b0 + n_box], p["boxes"], tabs["wb"][0], tabs["bb"][0], dtype=F32)
        print(line + " | d_wb err %.3e bound %.3e d_bb err %.3e bound %.3e fp32-yardstick %.3e" % (
            ew, tw, eb, tb, max(float((y32[0].double() - rw).abs().max()), float((y32[1].double() - rb).abs().max()))))


def dec_problem(O, n_attr, seed=0, rows=(7, 5)):
    g = GC._seed("dec", O, n_attr, seed)
    ro, ra = (r if r > 0 else v for r, v in zip(rows, (7, 5)))
    return dict(O=O, n_attr=n_attr, rows=rows, objs=ids(g, O, ro), attrs=ids(g, O, ra), obj_emb=GC._randn(g, ro, N_OBJ),
                attr_emb=GC._randn(g, ra, n_attr) if n_attr else None, mu=GC._randn(g, O, N_Z), logvar=0.5 * GC._randn(g, O, N_Z),
                eps=GC._randn(g, O, N_Z), z_in=GC._randn(g, O, N_Z), dx0=GC._randn(g, O, N_OBJ + n_attr + N_Z))


def dec_fwd_launch(L, p, form, z_in_x0, with_z):
    keep = []
    Wx = N_OBJ + p["n_attr"] + (N_Z if z_in_x0 else 0)
    x0 = torch.full((p["O"] + 1, Wx), SENT, device="cuda")
    z = torch.full((p["O"] + 1, N_Z), SENT, device="cuda")
    d = embed_desc(L, keep, kind=M_DEC, objs=_cu(p["objs"]), attrs=_cu(p["attrs"]), obj_emb=_cu(p["obj_emb"]),
                   attr_emb=None if p["attr_emb"] is None else _cu(p["attr_emb"]), mu=None if form == "z_in" else _cu(p["mu"]),
                   logvar=_cu(p["logvar"]) if form == "reparam" else None, eps=_cu(p["eps"]) if form == "reparam" else None,
                   z_in=_cu(p["z_in"]) if form == "z_in" else None, z=z if with_z else None, x0=x0, O=p["O"], n_obj=N_OBJ, n_attr=p["n_attr"], n_z=N_Z,
                   use_ae=int(form == "use_ae"), z_in_x0=z_in_x0)
    keep.append(d)
    return d, x0, z, keep


def dec_fwd_check(p, form, z_in_x0, with_z, x0, z, tag):
    O, b0 = p["O"], N_OBJ + p["n_attr"]
    gx, gz = x0.cpu(), z.cpu()
    _untouched(gx[O:], tag + ": x0 behind O")
    _untouched(gz[O:] if with_z else gz, tag + ": z behind O / a z that was not passed")
    assert torch.equal(gx[:O, :N_OBJ], p["obj_emb"][p["objs"]]), tag
    if p["n_attr"]:
        assert torch.equal(gx[:O, N_OBJ:b0], p["attr_emb"][p["attrs"]]), tag
    rz = {"z_in": p["z_in"].double(), "use_ae": p["mu"].double(), "reparam": V.reparam(p["mu"], p["logvar"], p["eps"])}[form]
    y = float((V.reparam(p["mu"], p["logvar"], p["eps"], dtype=F32).double() - rz).abs().max()) if form == "reparam" else 0.0
    for name, got in (("x0's z columns", gx[:O, b0:] if z_in_x0 else None), ("z", gz[:O] if with_z else None)):
        if got is None:
            continue
        if form == "reparam":
            e, tol = _assert_close(got, rz, 2e-6, 1e-6, tag + " " + name, form)
            print("%s %s: err %.3e bound %.3e fp32-yardstick %.3e" % (tag, name, e, tol, y))
        else:
            assert torch.equal(got.double(), rz), tag + ": " + name + " is a copy"


@pytest.mark.parametrize("form", ["z_in", "use_ae", "reparam"])
@pytest.mark.parametrize("O", [1, 65])
def test_dec_assemble(O, form):
    L = _lib()
    for n_attr in (0, N_ATTR):
        p = dec_problem(O, n_attr)
        for z_in_x0, with_z in ((1, 1), (1, 0), (0, 1)):
            d, x0, z, keep = dec_fwd_launch(L, p, form, z_in_x0, with_z)
            rc, _ = launch_embed(L, [d], what="dec_assemble " + form)
            assert rc == 0, rc
            dec_fwd_check(p, form, z_in_x0, with_z, x0, z, "dec_assemble[O=%d %s n_attr=%d z_in_x0=%d z=%d]" % (O, form, n_attr, z_in_x0, with_z))


def dec_bwd_launch(L, p, z_in_x0, with_dz):
    keep = []
    W = N_OBJ + p["n_attr"] + (N_Z if z_in_x0 else 0)
    tabs = asm_tables(p, ["obj_emb"] + (["attr_emb"] if p["n_attr"] else []))
    dz = torch.full((p["O"] + 1, N_Z), SENT, device="cuda")
    dx0 = p["dx0"][:, :W].contiguous()
    d = embed_desc(L, keep, kind=M_DEC_BWD, objs=_cu(p["objs"]), attrs=_cu(p["attrs"]), dx0=_cu(dx0), d_obj_emb=tabs["obj_emb"][1],
                   d_attr_emb=tabs["attr_emb"][1] if p["n_attr"] else None, dz=dz if with_dz else None, O=p["O"], n_obj=N_OBJ, n_attr=p["n_attr"], n_z=N_Z,
                   z_in_x0=z_in_x0, rows_obj=p["rows"][0], rows_attr=p["rows"][1])
    keep.append(d)
    return d, tabs, dz, dx0, keep


def dec_bwd_check(p, z_in_x0, with_dz, tabs, dz, dx0, tag, route):
    line = check_table(tabs["obj_emb"][1], tabs["obj_emb"][0], p["objs"], dx0, 0, N_OBJ, tag + " obj", route)
    if p["n_attr"]:
        line += " | " + check_table(tabs["attr_emb"][1], tabs["attr_emb"][0], p["attrs"], dx0, N_OBJ, p["n_attr"], tag + " attr", route)
    gz = dz.cpu()
    if z_in_x0 and with_dz:
        _untouched(gz[p["O"]:], tag + ": dz behind O")
        assert torch.equal(gz[:p["O"]], dx0[:, N_OBJ + p["n_attr"]:]), tag + ": dz is a copy"
    else:
        _untouched(gz, tag + ": dz with z_in_x0 = 0 / not passed")
    print(line)


DEC_ROUTES = {"lds": (7, 5), "plain-rows0": (0, 0), "plain-big": (1300, 5), "det": (7, 5)}


@pytest.mark.parametrize("route", list(DEC_ROUTES))
@pytest.mark.parametrize("O", ASM_OS)
def test_dec_assemble_bwd(O, route):
    L = _lib()
    for n_attr in (0, N_ATTR):
        p = dec_problem(O, n_attr, rows=DEC_ROUTES[route])
        for z_in_x0, with_dz in ((1, 1), (1, 0), (0, 1)):
            tag = "dec_assemble_bwd[O=%d %s n_attr=%d z_in_x0=%d dz=%d]" % (O, route, n_attr, z_in_x0, with_dz)
            runs = []
            with deterministic(L, route == "det"):
                for _ in range(2 if route == "det" else 1):
                    d, tabs, dz, dx0, keep = dec_bwd_launch(L, p, z_in_x0, with_dz)
                    rc, _ = launch_embed(L, [d], what=tag)
                    assert rc == 0, rc
                    runs.append([v[1].cpu() for v in tabs.values()])
            if route == "det":
                assert all(torch.equal(a, b) for a, b in zip(*runs)), tag + ": two deterministic runs differ"
            dec_bwd_check(p, z_in_x0, with_dz, tabs, dz, dx0, tag, route)


def embed_bwd_launch(L, kind, rows, n, table_rows_arg, seed=0, table_rows=12):
    g = GC._seed("embed-bwd", kind, rows, n, seed)
    idx = ids(g, rows, table_rows)
    d_src = GC._randn(g, rows, 8 + n + 3)                   # col0 = 8, ld > col0 + n
    t0 = GC._randn(g, table_rows, n)
    buf = sent_rows(t0)
    keep = []
    d = embed_desc(L, keep, kind=kind, idx=_cu(idx if kind == M_BWD_I64 else idx.int()), src=_cu(d_src), dst=buf, O=rows, n=n, ld=d_src.shape[1], col0=8,
                   table_rows=table_rows_arg)
    keep.append(d)
    return d, buf, t0, idx, d_src, keep


@pytest.mark.parametrize("route", ["lds", "plain-rows0", "plain-big", "det"])
@pytest.mark.parametrize("kind", [M_BWD_I32, M_BWD_I64], ids=["i32", "i64"])
def test_embed_bwd(kind, route):
    """d_emb[idx[r], :] += d[r, 8 : 8 + n] through the LDS route (table_rows * n <= 8 192), plain atomics (table_rows = 0, and a
    table above 8 192 floats) and the deterministic route (two runs bit-identical); the last table row is named by no index."""
    L = _lib()
    for rows in (1, 16, 17, 129):
        for n in (1, 64, 65):
            if route == "plain-big" and n == 1:
                continue                                   # 8 193 table rows of one float say nothing the n = 64 case does not
            trows = 130 if route == "plain-big" else 12    # 130 * 64 = 8 320 > 8 192
            arg = 0 if route == "plain-rows0" else trows
            tag = "embed_bwd[%s %s rows=%d n=%d]" % ("i64" if kind == M_BWD_I64 else "i32", route, rows, n)
            runs = []
            with deterministic(L, route == "det"):
                for _ in range(2 if route == "det" else 1):
                    d, buf, t0, idx, d_src, keep = embed_bwd_launch(L, kind, rows, n, arg, table_rows=trows)
                    rc, _ = launch_embed(L, [d], what=tag)
                    assert rc == 0, rc
                    runs.append(buf.cpu())
            if route == "det":
                assert torch.equal(runs[0], runs[1]), tag + ": two deterministic runs differ"
            print(check_table(buf, t0, idx, d_src, 8, n, tag, route))


def test_embed_gather_and_i64_to_i32_are_copies():
    L = _lib()
    for rows in (1, 129):
        g = GC._seed("gather", rows)
        idx = torch.randint(0, 9, (rows,), generator=g)
        k2, i32 = [], torch.full((rows + 1,), -7, dtype=torch.int32, device="cuda")
        rc, _ = launch_embed(L, [embed_desc(L, k2, kind=M_I64_I32, idx=_cu(idx), dst=i32, O=rows)], what="i64_to_i32")
        assert rc == 0 and torch.equal(i32.cpu()[:rows], idx.int()) and int(i32[rows]) == -7
        for n in (1, 65):
            emb = GC._randn(g, 9, n)
            keep, out = [], torch.full((rows + 1, n), SENT, device="cuda")
            rc, _ = launch_embed(L, [embed_desc(L, keep, kind=M_GATHER, idx=i32, src=_cu(emb), dst=out, O=rows, n=n)], what="embed_gather")
            assert rc == 0, rc
            got = out.cpu()
            _untouched(got[rows:], "embed_gather: the row behind")
            assert torch.equal(got[:rows], emb[idx]), "embed_gather rows=%d n=%d" % (rows, n)


@pytest.mark.parametrize("bad", [None, "objs", "attrs", "angles", "attrs-unused"])
def test_stage_batch_and_validate_ids(bad):
    """O = 300 is a second workgroup.  Copies are exact, deg is cleared, the error word collects 2 / 4 / 8; with no attribute
    vocabulary (rows_attr = 0) stage_batch does not look at the attribute ids."""
    L = _lib()
    for O in (1, 300):
        g = GC._seed("stage", O, bad)
        t = dict(objs=torch.randint(0, 7, (O,), generator=g), attrs=torch.randint(0, 5, (O,), generator=g), angles=torch.randint(0, 9, (O,), generator=g))
        want = 0
        if bad in ("objs", "attrs", "angles"):
            t[bad][O - 1] = {"objs": 7, "attrs": -1, "angles": 9}[bad]
            want = {"objs": 2, "attrs": 4, "angles": 8}[bad]
        ra = 5
        if bad == "attrs-unused":
            t["attrs"][0], ra = 99, 0
        boxes = torch.rand(O, 6, generator=g)
        i64 = lambda: torch.full((O + 1,), -7, dtype=torch.int64, device="cuda")
        st = dict(st_objs=i64(), st_attrs=i64(), st_angles=i64(), st_boxes=torch.full((O + 1, 6), SENT, device="cuda"),
                  attrs32=torch.full((O + 1,), -7, dtype=torch.int32, device="cuda"), deg=torch.full((O + 1,), 12345, dtype=torch.int32, device="cuda"))
        err = torch.tensor([0, -7], dtype=torch.int32, device="cuda")
        keep = []
        d = embed_desc(L, keep, kind=M_STAGE, objs=_cu(t["objs"]), attrs=_cu(t["attrs"]), angles=_cu(t["angles"]), boxes=_cu(boxes), err=err, O=O, box_dim=6,
                       rows_obj=7, rows_attr=ra, rows_angle=9, **st)
        rc, _ = launch_embed(L, [d], what="stage_batch")
        assert rc == 0, rc
        tag = "stage_batch[O=%d bad=%s]" % (O, bad)
        assert err.cpu().tolist() == [want, -7], (tag, err.cpu().tolist())
        for k in ("objs", "attrs", "angles"):
            got = st["st_" + k].cpu()
            assert torch.equal(got[:O], t[k]) and int(got[O]) == -7, tag + ": " + k
        assert torch.equal(st["attrs32"].cpu()[:O], t["attrs"].int()) and int(st["attrs32"][O]) == -7, tag
        assert st["deg"].cpu().tolist() == [0] * O + [12345], tag
        gb = st["st_boxes"].cpu()
        assert torch.equal(gb[:O], boxes), tag
        _untouched(gb[O:], tag + ": boxes behind O")
        if bad == "attrs-unused":
            continue                                       # validate_ids always looks at the attributes
        for with_angles in (1, 0):
            err2 = torch.tensor([0, -7], dtype=torch.int32, device="cuda")
            k2 = []
            d2 = embed_desc(L, k2, kind=M_VALIDATE, objs=_cu(t["objs"]), attrs=_cu(t["attrs"]), angles=_cu(t["angles"]) if with_angles else None, err=err2,
                            O=O, rows_obj=7, rows_attr=5, rows_angle=9)
            rc, _ = launch_embed(L, [d2], what="validate_ids")
            assert rc == 0, rc
            assert err2.cpu().tolist() == [want if (with_angles or bad != "angles") else 0, -7], (tag, with_angles, err2.cpu().tolist())


def test_multi_embedding_forms():
    """Room tables of the embedding group.  dec_assemble and embed_gather carry no atomics: bit-identical to each room's own
    launch.  The gradients are atomic sums: within the table bound of the reference.  Rooms whose planners choose different
    variants are refused, and so is dec_assemble_bwd in deterministic mode (the planner has no multi form there); nothing is written."""
    L = _lib()
    probs = [dec_problem(O, N_ATTR, seed=O) for O in (65, 1, 17)]
    singles = []
    for p in probs:
        d, x0, z, keep = dec_fwd_launch(L, p, "reparam", 1, 1)
        assert launch_embed(L, [d], what="dec_assemble single")[0] == 0
        singles.append((x0.cpu(), z.cpu()))
    built = [dec_fwd_launch(L, p, "reparam", 1, 1) for p in probs]
    rc, var = launch_embed(L, [b[0] for b in built], multi=1, what="dec_assemble_multi")
    assert rc == 0 and var == 0, (rc, var)
    for i, p in enumerate(probs):
        assert torch.equal(built[i][1].cpu(), singles[i][0]) and torch.equal(built[i][2].cpu(), singles[i][1]), "dec_assemble room %d differs from its own launch" % i
        dec_fwd_check(p, "reparam", 1, 1, built[i][1], built[i][2], "multi dec_assemble room %d" % i)
    # dec_assemble_bwd: LDS tables (variant 0) and plain atomics (variant 1)
    for rows, want in (((7, 5), 0), ((0, 0), 1)):
        ps = [dec_problem(O, N_ATTR, seed=O, rows=rows) for O in (65, 1, 17)]
        built = [dec_bwd_launch(L, p, 1, 1) for p in ps]
        rc, var = launch_embed(L, [b[0] for b in built], multi=1, what="dec_assemble_bwd_multi")
        assert rc == 0 and var == want, (rc, var)
        for i, p in enumerate(ps):
            dec_bwd_check(p, 1, 1, built[i][1], built[i][2], built[i][3], "multi dec_assemble_bwd room %d variant %d" % (i, want), "multi")
    mixed = [dec_bwd_launch(L, dec_problem(17, N_ATTR, rows=r), 1, 1) for r in ((7, 5), (0, 0))]
    assert launch_embed(L, [b[0] for b in mixed], multi=1, what="dec_assemble_bwd_multi mixed")[0] == -2
    with deterministic(L, True):
        assert launch_embed(L, [mixed[0][0]], multi=1, what="dec_assemble_bwd_multi deterministic")[0] == -2
    for b in mixed:
        assert all(torch.equal(v[1].cpu()[:-1], v[0]) for v in b[1].values()), "a refused room set wrote a table"
        _untouched(b[2].cpu(), "dz of a refused room set")
    # embed_gather
    g = GC._seed("multi-gather")
    rooms = []
    for rows in (129, 1, 17):
        idx, emb = torch.randint(0, 9, (rows,), generator=g).int(), GC._randn(g, 9, 65)
        keep, out = [], torch.full((rows + 1, 65), SENT, device="cuda")
        rooms.append((embed_desc(L, keep, kind=M_GATHER, idx=_cu(idx), src=_cu(emb), dst=out, O=rows, n=65), out, emb[idx.long()], keep))
    rc, var = launch_embed(L, [r[0] for r in rooms], multi=1, what="embed_gather_multi")
    assert rc == 0 and var == 0, (rc, var)
    for d, out, ref, keep in rooms:
        got = out.cpu()
        _untouched(got[-1:], "embed_gather_multi: the row behind")
        assert torch.equal(got[:-1], ref)
    # embed_bwd: LDS (1 / 5), plain (2 / 6), deterministic (0 / 4)
    for kind, w in ((M_BWD_I32, 0), (M_BWD_I64, 4)):
        for arg, det, want in ((12, False, 1), (0, False, 2), (12, True, 0)):
            built = [embed_bwd_launch(L, kind, rows, 65, arg, seed=rows) for rows in (129, 1, 17)]
            with deterministic(L, det):
                rc, var = launch_embed(L, [b[0] for b in built], multi=1, what="embed_bwd_multi")
            assert rc == 0 and var == w + want, (rc, var, w + want)
            for i, (d, buf, t0, idx, d_src, keep) in enumerate(built):
                print(check_table(buf, t0, idx, d_src, 8, 65, "multi embed_bwd room %d variant %d" % (i, var), "multi"))
        mixed = [embed_bwd_launch(L, kind, 17, 65, arg) for arg in (12, 0)]
        assert launch_embed(L, [b[0] for b in mixed], multi=1, what="embed_bwd_multi mixed")[0] == -2
        for b in mixed:
            assert torch.equal(b[1].cpu()[:-1], b[2]), "a refused room set wrote a table"


# ================================================================================================= the step prologue
@pytest.mark.parametrize("zero_bytes", [0, 16, 4112])
@pytest.mark.parametrize("with_eps", [1, 0])
def test_step_prologue_is_its_four_launches(with_eps, zero_bytes):
    """One launch against the separate ones (the draw, enc_assemble, two predicate gathers, a cleared region): every output
    bit-identical.  eps NULL: no draw and the rng offset stays; otherwise it advances ONCE per launch.  zero_ptr NULL
    (zero_bytes 0 here), 16 bytes, and 4 112 = 257 sixteen-byte words: a second workgroup with one live lane."""
    L = _lib()
    g = GC._seed("prologue")
    O, T, n_eps, n_ec, n_dc = 65, 33, 1025, 65, 8
    p = enc_problem(O, N_ATTR, 65, 6)
    pidx = torch.randint(0, 9, (T,), generator=g).int()
    pemb_ec, pemb_dc = GC._randn(g, 9, n_ec), GC._randn(g, 9, n_dc)
    # the separate launches
    eps_s = torch.full((n_eps + 1,), SENT, device="cuda")
    run_opt(L, kind=1, params=eps_s, n=n_eps, seed=RANDN_SEED, offset=RANDN_OFFSET, calls=1)
    keep, x0_s = [], torch.full((O + 1, p["W"]), SENT, device="cuda")
    assert launch_embed(L, [enc_fwd_desc(L, p, keep, x0_s)], what="enc_assemble")[0] == 0
    outs_s = []
    for emb, n in ((pemb_ec, n_ec), (pemb_dc, n_dc)):
        o = torch.full((T + 1, n), SENT, device="cuda")
        assert launch_embed(L, [embed_desc(L, keep, kind=M_GATHER, idx=_cu(pidx), src=_cu(emb), dst=o, O=T, n=n)], what="embed_gather")[0] == 0
        outs_s.append(o.cpu())
    # the one launch
    for calls in (1, 2):
        eps = torch.full((n_eps + 1,), SENT, device="cuda")
        x0 = torch.full((O + 1, p["W"]), SENT, device="cuda")
        p0e, p0d = torch.full((T + 1, n_ec), SENT, device="cuda"), torch.full((T + 1, n_dc), SENT, device="cuda")
        region = torch.full((zero_bytes + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        assert region.data_ptr() % 16 == 0
        k2 = []
        pro = enc_fwd_desc(L, p, k2, x0)
        pidx_d, ec_d, dc_d = _cu(pidx), _cu(pemb_ec), _cu(pemb_dc)
        pro.idx, pro.src, pro.dst, pro.src2, pro.dst2 = _p(pidx_d), _p(ec_d), _p(p0e), _p(dc_d), _p(p0d)
        pro.T, pro.n, pro.n2 = T, n_ec, n_dc
        pro.zero_ptr, pro.zero_bytes = (_p(region), zero_bytes) if zero_bytes else (None, 0)
        d = run_opt(L, kind=2, params=eps if with_eps else None, n=n_eps if with_eps else 0, pro=C.pointer(pro), seed=RANDN_SEED,
                    offset=RANDN_OFFSET - (calls - 1), calls=calls)
        tag = "step_prologue[eps=%d zero_bytes=%d calls=%d]" % (with_eps, zero_bytes, calls)
        assert d.out_offset == RANDN_OFFSET - (calls - 1) + (calls if with_eps else 0), (tag, d.out_offset)
        if with_eps:
            assert torch.equal(eps.cpu(), eps_s.cpu()), tag + ": eps differs from sln_launch_randn at the same offset"
        else:
            _untouched(eps.cpu(), tag + ": eps")
        assert torch.equal(x0.cpu(), x0_s.cpu()), tag + ": x0 differs from enc_assemble"
        assert torch.equal(p0e.cpu(), outs_s[0]) and torch.equal(p0d.cpu(), outs_s[1]), tag + ": a predicate gather differs from embed_gather"
        r = region.cpu()
        assert bool((r[:zero_bytes] == 0).all()) and bool((r[zero_bytes:] == 0x5A).all()), tag + ": the cleared region"


# ================================================================================================= refusals, lab switches
def test_hooks_refuse_what_the_launchers_assume_without_launching():
    L = _lib()
    p = scatter_fwd_problem(L, 128, 8, "train", 5)
    d, out, keep = scatter_fwd_launch(L, p)
    for field, val in (("lda", 2 * 128 + 4), ("rows", p["O"] + 1), ("out", None), ("H", 0)):
        bad = L.SlnDbgEdge.from_buffer_copy(d)
        setattr(bad, field, val)
        assert launch_edge(L, [bad], what="refusal")[0] == -1, field
    bad = L.SlnDbgEdge.from_buffer_copy(d)
    bad.bn.cstride = 2 * 128 + 8 - 1
    assert launch_edge(L, [bad], what="refusal")[0] == -1
    assert launch_edge(L, [d, d], multi=0, what="refusal")[0] == -1
    _untouched(out.cpu(), "output of refused launches")
    assert L.lib().sln_debug_vae_loss(C.byref(loss_desc(L, kind=0, O=3)), L.current_stream_ptr()) == -1
    assert L.lib().sln_debug_vae_tables(2, (L.SlnDbgTranspose * 1)(), 1, 1, 0.0, 0, 0, 0, L.current_stream_ptr()) == -1
    o = L.SlnDbgOpt(); o.kind, o.n, o.calls = 0, 4, 1
    assert L.lib().sln_debug_vae_opt(C.byref(o), L.current_stream_ptr()) == -1
    o.kind = 2                                                    # a prologue without its description
    assert L.lib().sln_debug_vae_opt(C.byref(o), L.current_stream_ptr()) == -1
    d, buf, t0, idx, d_src, keep = embed_bwd_launch(L, M_BWD_I32, 17, 65, 12)
    for field, val in (("ld", 8 + 65 - 1), ("O", 0), ("dst", None), ("n", 0), ("kind", 10)):
        bad = L.SlnDbgEmbed.from_buffer_copy(d)
        setattr(bad, field, val)
        assert launch_embed(L, [bad], what="refusal")[0] == -1, field
    assert launch_embed(L, [d, d], multi=0, what="refusal")[0] == -1
    assert torch.equal(buf.cpu()[:-1], t0), "table of refused launches"
    torch.cuda.synchronize()


@pytest.mark.parametrize("env,val,k", [("SLN_SCATTER_NIT", "4", "test_scatter_avg_bwd"), ("SLN_GATHER_YT", "8", "test_gather_bwd"),
                                       ("SLN_GATHER_YT", "32", "test_gather_bwd")], ids=["scatter-nit4", "gather-yt8", "gather-yt32"])
def test_lab_switches_select_kernels_that_pass_the_same_cases(env, val, k):
    """SLN_SCATTER_NIT = 4 and SLN_GATHER_YT = 8 / 32 select other instantiations of shipped kernels (read once per process: a
    fresh child).  SLN_EDGE_ABL is not exercised: it skips launches by design.  The child's selection leaves this test out."""
    e = dict(os.environ); e[env] = val
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", k + " and not lab_switches"],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "deselected" in r.stdout, r.stdout[-500:]
