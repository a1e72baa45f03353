"""Plain reference of the fused GEMM family (csrc/gemm_f32.hip), written from the formulas in csrc/sln_common.h / sln_gemm.h.

Problems are described by the small record types below, holding CPU tensors (fp32 data, fp64 statistics, int32 indices).  Every
function takes ``dtype``: torch.float64 is the reference; torch.float32 evaluates the SAME formulas the way the kernels round
them (statistics reduced in fp64, coefficients and products in fp32) - its distance from the fp64 result is the yardstick for
what fp32 arithmetic can deliver on a transformed operand.  No kernel code path is involved.
"""
import torch

BN_NONE, BN_TRAIN, BN_EVAL = 0, 1, 2
COEF_IDENT, COEF_FWD, COEF_FWD_NORELU, COEF_BWD = 0, 1, 2, 3
EPI_PLAIN, EPI_STATS, EPI_MASK = 0, 1, 2
NEG = -3.0e38


class Rec:
    _defaults = {}

    def __init__(self, **kw):
        bad = set(kw) - set(self._defaults)
        assert not bad, bad
        for k, v in self._defaults.items():
            setattr(self, k, kw.get(k, v))

    def replace(self, **kw):
        d = {k: getattr(self, k) for k in self._defaults}
        d.update(kw)
        return type(self)(**d)


class Bn(Rec):
    """BatchNorm view aligned with the first column of what it normalises.  sums / gsums: [2, C] fp64."""
    _defaults = dict(mode=BN_NONE, gamma=None, beta=None, rmean=None, rvar=None, sums=None, gsums=None, n_rows=1.0, eps=1e-5)


class Seg(Rec):
    """len logical columns: x1[:, c1:c1+len] (and x2[:, c2:c2+len]); which: 0 plain rows, 1 rows idx_a, 2 rows idx_b."""
    _defaults = dict(x1=None, c1=0, x2=None, c2=0, len=0, which=0, coef=COEF_IDENT, bn=None)


class Operand(Rec):
    _defaults = dict(segs=(), idx_a=None, idx_b=None)


class NT(Rec):
    """Y[:, ycol0:ycol0+N] = op(A) W[:, :K]^T + bias + addend[:, addcol0:addcol0+N]; xprev / obn: the masked epilogue."""
    _defaults = dict(A=None, W=None, bias=None, M=0, N=0, K=0, ldy=0, ycol0=0, addend=None, addcol0=0, epi=EPI_PLAIN,
                     xprev=None, xcol0=0, obn=None, tile=-1, ocstride=0)


class TN(Rec):
    """dW[:, :Kin] += op(G)^T op(X), db += colsum(op(G)); sgd_step (a float): the parameters receive -step * gradient."""
    _defaults = dict(G=None, X=None, R=0, Nout=0, Kin=0, dW0=None, db0=None, sgd_step=None, rows_per_block=0)


# ------------------------------------------------------------------------------------------------ BatchNorm coefficients
def sums_of(x):
    """[2, C] fp64 column sums of x and x^2 over all rows of x."""
    xd = x.double()
    return torch.stack([xd.sum(0), (xd * xd).sum(0)])


def mean_istd(bn, C, dtype):
    if bn is None or bn.mode == BN_NONE:
        return torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype)
    eps = torch.tensor(bn.eps, dtype=torch.float32).to(dtype)
    if bn.mode == BN_TRAIN:
        rn = 1.0 / float(bn.n_rows)
        m = bn.sums[0, :C].double() * rn
        v = (bn.sums[1, :C].double() * rn - m * m).clamp_min(0.0)      # variance clamped at 0
        return m.to(dtype), 1.0 / torch.sqrt(v.to(dtype) + eps)
    return bn.rmean[:C].to(dtype), 1.0 / torch.sqrt(bn.rvar[:C].to(dtype) + eps)


def fwd_coef(bn, C, dtype):
    """(scale, shift, mean, istd): h = scale * x + shift."""
    mean, istd = mean_istd(bn, C, dtype)
    if bn is None or bn.mode == BN_NONE:
        return torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype), mean, istd
    scale = bn.gamma[:C].to(dtype) * istd
    return scale, bn.beta[:C].to(dtype) - mean * scale, mean, istd


def bwd_coef(bn, C, dtype):
    """dX = p0 * g + p1 * x + p2 (g: the ReLU-masked gradient w.r.t. the BatchNorm output, x: the pre-activation)."""
    one, zero = torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype)
    if bn is None or bn.mode == BN_NONE:
        return one, zero, zero
    mean, istd = mean_istd(bn, C, dtype)
    scale = bn.gamma[:C].to(dtype) * istd
    if bn.mode == BN_EVAL:
        return scale, zero, zero
    rn = 1.0 / float(bn.n_rows)
    c1 = (bn.gsums[0, :C].double() * rn).to(dtype)
    c2 = (bn.gsums[1, :C].double() * rn).to(dtype)
    p1 = -scale * istd * c2
    return scale, p1, -scale * c1 - p1 * mean


def seg_coefs(seg, dtype):
    """(c0, c1, c2, floor) per column: v = max(c0 * x1 + c1 * x2 + c2, floor)."""
    C = seg.len
    one, zero, neg = torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype), torch.full((C,), NEG, dtype=dtype)
    if seg.coef == COEF_IDENT:
        return one, zero, zero, neg
    if seg.coef == COEF_BWD:
        p0, p1, p2 = bwd_coef(seg.bn, C, dtype)
        return p0, p1, p2, neg
    scale, shift, _, _ = fwd_coef(seg.bn, C, dtype)
    return scale, zero, shift, (zero if seg.coef == COEF_FWD else neg)


# ------------------------------------------------------------------------------------------------ operand, NT, TN
def operand(op, rows, dtype=torch.float64):
    """The logical [rows, sum of lens] operand."""
    out = []
    for s in op.segs:
        if s.which == 0:
            r = torch.arange(rows)
        else:
            r = (op.idx_a if s.which == 1 else op.idx_b)[:rows].long()
        c0, c1, c2, floor = seg_coefs(s, dtype)
        v = c0 * s.x1[r, s.c1:s.c1 + s.len].to(dtype) + c2
        if s.x2 is not None:
            v = v + c1 * s.x2[r, s.c2:s.c2 + s.len].to(dtype)
        out.append(torch.maximum(v, floor))
    return torch.cat(out, 1)


def nt(p, dtype=torch.float64):
    """-> dict(y [M, N], sums [2, N] or None (EPI_STATS: sum y, sum y^2; EPI_MASK: sum g, sum g * xhat))."""
    A = operand(p.A, p.M, dtype)
    assert A.shape == (p.M, p.K)
    y = A @ p.W[:p.N, :p.K].to(dtype).t()
    if p.bias is not None:
        y = y + p.bias[:p.N].to(dtype)
    if p.addend is not None:
        y = y + p.addend[:p.M, p.addcol0:p.addcol0 + p.N].to(dtype)
    sums = None
    if p.epi == EPI_STATS:
        yd = y.double()
        sums = torch.stack([yd.sum(0), (yd * yd).sum(0)])
    elif p.epi == EPI_MASK:
        xp = p.xprev[:p.M, p.xcol0:p.xcol0 + p.N].to(dtype)
        scale, shift, mean, istd = fwd_coef(p.obn, p.N, dtype)
        y = y * (scale * xp + shift > 0).to(dtype)
        sums = torch.stack([y.double().sum(0), (y * ((xp - mean) * istd)).double().sum(0)])
    return dict(y=y, sums=sums)


def tn(p, dtype=torch.float64):
    """-> (dW [Nout, Kin], db [Nout] or None): the final contents of the accumulated-into buffers."""
    G = operand(p.G, p.R, dtype)
    X = operand(p.X, p.R, dtype)
    assert G.shape == (p.R, p.Nout) and X.shape == (p.R, p.Kin)
    f = 1.0 if p.sgd_step is None else -float(torch.tensor(p.sgd_step, dtype=torch.float32))
    dW = p.dW0[:, :p.Kin].to(dtype) + f * (G.t() @ X)
    db = None if p.db0 is None else p.db0.to(dtype) + f * G.sum(0)
    return dW, db


# ------------------------------------------------------------------------------------------------ thresholds
def mask_margin(xprev, obn):
    """min over elements of |scale * xprev + shift| / (spread of its column), fp64."""
    scale, shift, _, _ = fwd_coef(obn, xprev.shape[1], torch.float64)
    z = scale * xprev.double() + shift
    spread = z.std(0, unbiased=False).clamp_min(1e-30)
    return float((z.abs() / spread).min())


def condition_mask(xprev, make_bn, margin=1e-3, max_iter=20):
    """Move the entries of xprev whose scale * x + shift lies within `margin` of its column's spread away from the threshold
    (EPI_MASK is discontinuous there: an fp32 and an fp64 evaluation may legitimately disagree).  make_bn(xprev) rebuilds the
    BatchNorm view - train-mode statistics depend on xprev itself - so the loop repeats until no entry offends.
    Returns (xprev, bn); no element is excluded from any later comparison."""
    xprev = xprev.clone()
    for _ in range(max_iter):
        bn = make_bn(xprev)
        scale, shift, _, _ = fwd_coef(bn, xprev.shape[1], torch.float64)
        z = scale * xprev.double() + shift
        spread = z.std(0, unbiased=False)
        bad = z.abs() < margin * spread
        if not bool(bad.any()):
            return xprev, bn
        sgn = torch.where(z >= 0, 1.0, -1.0)
        # put the offender at 8 margins from the threshold, on the side it was on
        target = sgn * 8.0 * margin * spread
        xnew = ((target - shift) / scale).float()
        xprev = torch.where(bad, xnew, xprev)
    raise AssertionError("could not move xprev away from the mask threshold")
