"""The GEMM-family suite's own footing, checkable without a GPU: the fp64 reference (tests/gemm_ref.py) against torch itself, the
ctypes mirrors of the hook descriptions against the C layout, and the body every listed shape of the GPU case table reaches."""
import ctypes as C

import pytest
import torch

from conftest import pkg
import gemm_cases as GC
import gemm_ref as R


def _bn_module(bn, C_, training):
    m = torch.nn.BatchNorm1d(C_, eps=bn.eps).double()
    with torch.no_grad():
        m.weight.copy_(bn.gamma.double()); m.bias.copy_(bn.beta.double())
        if bn.mode == R.BN_EVAL:
            m.running_mean.copy_(bn.rmean.double()); m.running_var.copy_(bn.rvar.double())
    return m.train(training)


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_forward_operand_is_relu_batchnorm(mode):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(37, 24, generator=g) * 1.7 + 0.4
    view = x[:, 4:20]
    bn = GC.bn_train(g, view) if mode == "train" else GC.bn_eval(g, 16)
    op = R.Operand(segs=(R.Seg(x1=x, c1=4, len=16, coef=R.COEF_FWD, bn=bn),))
    want = torch.relu(_bn_module(bn, 16, mode == "train")(view.double()))
    torch.testing.assert_close(R.operand(op, 37), want, rtol=1e-12, atol=1e-12)
    # without the ReLU
    op2 = R.Operand(segs=(R.Seg(x1=x, c1=4, len=16, coef=R.COEF_FWD_NORELU, bn=bn),))
    torch.testing.assert_close(R.operand(op2, 37), _bn_module(bn, 16, mode == "train")(view.double()), rtol=1e-12, atol=1e-12)


def test_backward_operand_is_autograd_through_relu_batchnorm():
    """y = EPI_MASK(dh W^T): the gradient w.r.t. bn(x) of h = relu(bn(x)) and the sums it leaves behind; the SLN_COEF_BWD
    operand built from them is autograd's gradient w.r.t. x."""
    g = torch.Generator().manual_seed(2)
    Mr, N, K = 29, 12, 8
    x = (torch.randn(Mr, N, generator=g) + 0.3)
    gamma, beta = GC._uniform(g, N, 0.5, 1.5), 0.5 * torch.randn(N, generator=g)
    xv, obn = R.condition_mask(x, lambda t: R.Bn(mode=R.BN_TRAIN, gamma=gamma, beta=beta, sums=R.sums_of(t), n_rows=float(Mr)))
    dh_src = torch.randn(Mr, K, generator=g)          # gradient arriving at the next Linear's output
    Wt = torch.randn(N, K, generator=g)               # that Linear's weight, transposed for the dgrad
    p = R.NT(A=R.Operand(segs=(R.Seg(x1=dh_src, len=K),)), W=Wt, M=Mr, N=N, K=K, ldy=N, epi=R.EPI_MASK, xprev=xv, obn=obn, ocstride=N)
    out = R.nt(p)
    gmask = out["y"]
    bwd = R.Bn(mode=R.BN_TRAIN, gamma=gamma, beta=beta, sums=obn.sums, gsums=out["sums"], n_rows=float(Mr))
    dx = R.operand(R.Operand(segs=(R.Seg(x1=gmask.float(), x2=xv, len=N, coef=R.COEF_BWD, bn=bwd),)), Mr)
    # autograd
    xa = xv.double().requires_grad_(True)
    h = torch.relu(_bn_module(obn, N, True)(xa))
    (h * (dh_src.double() @ Wt.double().t())).sum().backward()
    # (gmask went through fp32 on its way into the operand: 1e-7 relative)
    torch.testing.assert_close(dx, xa.grad, rtol=0, atol=2e-6 * float(xa.grad.abs().max()))
    # and with the fp64 gradient itself, exactly
    x1 = gmask
    p0, p1, p2 = R.bwd_coef(bwd, N, torch.float64)
    torch.testing.assert_close(p0 * x1 + p1 * xv.double() + p2, xa.grad, rtol=1e-11, atol=1e-12)


def test_gathered_concat_operand_is_torch_cat():
    g = torch.Generator().manual_seed(3)
    obj, pred = torch.randn(9, 32, generator=g), torch.randn(20, 64, generator=g)
    s, o = GC.gather_index(g, 20, 9), GC.gather_index(g, 20, 9)
    assert (s[1:] < s[:-1]).any() and len(set(s.tolist())) < 20          # non-monotone, with repeats
    op = R.Operand(segs=(R.Seg(x1=obj, len=32, which=1), R.Seg(x1=pred, len=64), R.Seg(x1=obj, len=32, which=2)), idx_a=s, idx_b=o)
    want = torch.cat([obj[s.long()], pred, obj[o.long()]], 1).double()
    assert torch.equal(R.operand(op, 20), want)


def test_nt_and_tn_reference_are_matmuls():
    g = torch.Generator().manual_seed(4)
    x, W, b, add = torch.randn(11, 8, generator=g), torch.randn(5, 8, generator=g), torch.randn(5, generator=g), torch.randn(11, 9, generator=g)
    p = R.NT(A=R.Operand(segs=(R.Seg(x1=x, len=8),)), W=W, bias=b, addend=add, addcol0=2, M=11, N=5, K=8, ldy=5, epi=R.EPI_STATS, ocstride=5)
    out = R.nt(p)
    y = x.double() @ W.double().t() + b.double() + add[:, 2:7].double()
    torch.testing.assert_close(out["y"], y, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(out["sums"], torch.stack([y.sum(0), (y * y).sum(0)]), rtol=1e-13, atol=1e-13)
    gq, dW0, db0 = torch.randn(11, 4, generator=g), torch.randn(4, 8, generator=g), torch.randn(4, generator=g)
    t = R.TN(G=R.Operand(segs=(R.Seg(x1=gq, len=4),)), X=R.Operand(segs=(R.Seg(x1=x, len=8),)), R=11, Nout=4, Kin=8, dW0=dW0, db0=db0)
    dW, db = R.tn(t)
    torch.testing.assert_close(dW, dW0.double() + gq.double().t() @ x.double(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(db, db0.double() + gq.double().sum(0), rtol=1e-13, atol=1e-13)
    dW2, db2 = R.tn(t.replace(sgd_step=0.25))
    torch.testing.assert_close(dW2, dW0.double() - 0.25 * (gq.double().t() @ x.double()), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(db2, db0.double() - 0.25 * gq.double().sum(0), rtol=1e-13, atol=1e-13)


def test_description_structs_match_the_c_layout():
    L = pkg("_lib")
    out = (C.c_int * 6)()
    assert L.lib().sln_debug_gemm_sizes(out, 6) == 6
    mirrors = (L.SlnDbgBn, L.SlnDbgSeg, L.SlnDbgOperand, L.SlnDbgGemmNT, L.SlnDbgGemmTN, L.SlnDbgNTRoute)
    assert list(out) == [C.sizeof(m) for m in mirrors]


@pytest.mark.parametrize("case", GC.nt_cases(), ids=GC.nt_case_id)
def test_listed_shape_reaches_its_body(case):
    L = pkg("_lib")
    (name, body, multi, M, N, K, lens, tile), mode, epi, _ = case
    p = GC.nt_case_problem(case)
    want_threads = 512 if body not in (GC.B128x64, GC.B128) and (mode != "ident" or epi == R.EPI_MASK) else 256
    for q in (p, p.replace(bias=None, addend=None)):
        got = GC.route(L, q)
        assert got == (body, multi, GC.AMODE_OF[mode], want_threads), "%s routes to %s" % (name, GC.route_text(got))


def test_route_hook_rejects_what_the_engine_never_builds():
    L = pkg("_lib")
    p = GC.nt_case_problem(GC.nt_cases()[0])

    def rc(mut):
        d = GC.nt_desc(L, p, GC.fake_ptr, Y=1, osums=1)
        mut(d)
        return L.lib().sln_debug_gemm_nt_route(C.byref(d), C.byref(L.SlnDbgNTRoute()))
    assert rc(lambda d: None) == 0
    assert rc(lambda d: setattr(d.A.seg[0], "len", 34)) == -1            # not a multiple of 4
    assert rc(lambda d: setattr(d, "K", 40)) == -1                       # K is the sum of the lens
    assert rc(lambda d: setattr(d, "W", None)) == -1
    assert rc(lambda d: setattr(d.A.seg[0], "which", 1)) == -1           # gathered without an index array
    assert rc(lambda d: setattr(d.A.seg[0], "ld1", d.A.seg[0].ld1 + 2)) == -1   # rows are read as float4
    assert rc(lambda d: setattr(d, "ldy", d.N)) == -1                    # the output window must fit its rows
