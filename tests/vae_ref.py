"""Plain reference of the non-GEMM kernels of the VAE path (csrc/vae_kernels.hip), written from the comments of csrc/vae_kernels.h
and the formulas of csrc/sln_common.h.  CPU tensors in, CPU tensors out; no kernel code path is involved.

Every function takes ``dtype``: torch.float64 is the reference, torch.float32 evaluates the SAME formulas in the precision the
kernels work in (statistics still reduced in fp64) - its distance from the fp64 result is the yardstick the GPU suite prints.
BatchNorm views are gemm_ref.Bn records aligned with the first column of what they normalise.
"""
import numpy as np
import torch

from gemm_ref import BN_NONE, BN_TRAIN, BN_EVAL, Bn, fwd_coef, mean_istd, mask_margin, condition_mask, sums_of   # noqa: F401 (re-exported)


# ------------------------------------------------------------------------------------------------ graph CSR
def csr(tri, O, num_preds, edges_only=False):
    """tri: int64 [T, 3] (s, p, o) or [T, 2] (s, o).  -> dict(s, p, o int32 [T]; deg int32 [O]; rowptr int64 [O + 1];
    rows: list of ascending entry lists (entry e < T: triple e as subject, e >= T: triple e - T as object); err)."""
    T = tri.shape[0]
    s = tri[:, 0].clone() if T else torch.zeros(0, dtype=torch.int64)
    o = tri[:, -1].clone() if T else torch.zeros(0, dtype=torch.int64)
    p = torch.zeros(T, dtype=torch.int64) if edges_only or not T else tri[:, 1].clone()
    bad = (s < 0) | (s >= O) | (o < 0) | (o >= O) | (p < 0) | (p >= (1 if edges_only else num_preds))
    s[bad] = 0; p[bad] = 0; o[bad] = 0          # an out-of-range triple is flagged and neutralised to (0, 0, 0)
    deg = torch.zeros(O, dtype=torch.int64)
    rows = [[] for _ in range(O)]
    for e in range(T):
        rows[int(s[e])].append(e)
    for e in range(T):
        rows[int(o[e])].append(T + e)
    for i in range(O):
        deg[i] = len(rows[i])
    rowptr = torch.zeros(O + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    return dict(s=s.int(), p=p.int(), o=o.int(), deg=deg.int(), rowptr=rowptr, rows=rows, err=1 if bool(bad.any()) else 0)


def invdeg(deg, dtype=torch.float64):
    return 1.0 / deg.clamp_min(1).to(dtype)


# ------------------------------------------------------------------------------------------------ edge kernels
def _act(x, bn, dtype):
    """relu(bn(x)), the mask [bn(x) > 0] and xhat = (x - mean) * istd of the pre-activation x [rows, C]"""
    scale, shift, mean, istd = fwd_coef(bn, x.shape[1], dtype)
    z = scale * x.to(dtype) + shift
    return z.clamp_min(0), (z > 0).to(dtype), (x.to(dtype) - mean) * istd


def _gsums(g, xhat):
    return torch.stack([g.double().sum(0), (g * xhat).double().sum(0)])


def scatter_avg_fwd(A2, H, D, bn, s, o, O, dtype=torch.float64):
    """pooled[i] = (sum_{t: s_t = i} h[t, :H] + sum_{t: o_t = i} h[t, H + D:]) / max(deg_i, 1), h = relu(bn(A2[:, :2H + D]))"""
    h, _, _ = _act(A2[:, :2 * H + D], bn, dtype)
    pooled = torch.zeros(O, H, dtype=dtype)
    pooled.index_add_(0, s.long(), h[:, :H])
    pooled.index_add_(0, o.long(), h[:, H + D:])
    deg = torch.zeros(O, dtype=torch.int64)
    deg.index_add_(0, s.long(), torch.ones_like(s, dtype=torch.int64))
    deg.index_add_(0, o.long(), torch.ones_like(o, dtype=torch.int64))
    return pooled * invdeg(deg, dtype)[:, None]


def scatter_avg_bwd(dM, dP, dpcol0, A2, H, D, bn, s, o, dtype=torch.float64):
    """g2 = mask(bn(A2)) * [dM[s] / deg_s | dP[:, dpcol0 : dpcol0 + D] (0 without dP) | dM[o] / deg_o]; -> (g2, gsums [2, 2H + D])"""
    O, T = dM.shape[0], A2.shape[0]
    deg = torch.zeros(O, dtype=torch.int64)
    deg.index_add_(0, s.long(), torch.ones(T, dtype=torch.int64))
    deg.index_add_(0, o.long(), torch.ones(T, dtype=torch.int64))
    w = invdeg(deg, dtype)[:, None]
    dMw = dM[:, :H].to(dtype) * w
    mid = torch.zeros(T, D, dtype=dtype) if dP is None else dP[:, dpcol0:dpcol0 + D].to(dtype)
    d = torch.cat([dMw[s.long()], mid, dMw[o.long()]], 1)
    _, mask, xhat = _act(A2[:, :2 * H + D], bn, dtype)
    g2 = d * mask
    return g2, _gsums(g2, xhat)


def gather_bwd(dG, D, s, o, O, add1, xprev, bn, masked, dtype=torch.float64):
    """dX[i] = sum_{t: s_t = i} dG[t, :D] + sum_{t: o_t = i} dG[t, 2D : 3D] + add1[i]; masked: times [bn(xprev) > 0], with gsums"""
    d = torch.zeros(O, D, dtype=dtype)
    d.index_add_(0, s.long(), dG[:, :D].to(dtype))
    d.index_add_(0, o.long(), dG[:, 2 * D:3 * D].to(dtype))
    if add1 is not None:
        d = d + add1[:, :D].to(dtype)
    if not masked:
        return d, None
    _, mask, xhat = _act(xprev[:, :D], bn, dtype)
    d = d * mask
    return d, _gsums(d, xhat)


def mask_gstats(d1, d2, xprev, bn, rows, cols, dtype=torch.float64):
    d = d1[:rows, :cols].to(dtype)
    if d2 is not None:
        d = d + d2[:rows, :cols].to(dtype)
    _, mask, xhat = _act(xprev[:rows, :cols], bn, dtype)
    d = d * mask
    return d, _gsums(d, xhat)


def bn_relu_apply(x, col0, cols, bn, dtype=torch.float64):
    return _act(x[:, col0:col0 + cols], bn, dtype)[0]


# ------------------------------------------------------------------------------------------------ embeddings, reparameterisation
def enc_assemble(objs, attrs, angles, boxes, obj_emb, attr_emb, angle_emb, wb, bb, dtype=torch.float64):
    """X0 = [obj_emb[objs] | attr_emb[attrs] | boxes Wb^T + bb | angle_emb[angles]] (attr_emb None: no attribute columns)"""
    parts = [obj_emb.to(dtype)[objs]]
    if attr_emb is not None:
        parts.append(attr_emb.to(dtype)[attrs])
    parts.append(boxes.to(dtype) @ wb.to(dtype).t() + bb.to(dtype))
    parts.append(angle_emb.to(dtype)[angles])
    return torch.cat(parts, 1)


def embed_bwd(idx, d, col0, n, table0, dtype=torch.float64):
    """table0 + (rows of d[:, col0 : col0 + n] added onto rows idx)"""
    out = table0.to(dtype).clone()
    out.index_add_(0, idx.long(), d[:, col0:col0 + n].to(dtype))
    return out


def box_linear_bwd(dx, boxes, dwb0, dbb0, dtype=torch.float64):
    """the box Linear's gradients, accumulated: d_wb += dx^T boxes, d_bb += colsum(dx)"""
    return dwb0.to(dtype) + dx.to(dtype).t() @ boxes.to(dtype), dbb0.to(dtype) + dx.to(dtype).sum(0)


def reparam(mu, logvar, eps, dtype=torch.float64):
    return eps.to(dtype) * torch.exp(0.5 * logvar.to(dtype)) + mu.to(dtype)


# ------------------------------------------------------------------------------------------------ loss
def log_softmax(x, dtype=torch.float64):
    x = x.to(dtype)
    m = x.max(1, keepdim=True).values
    return x - (torch.log(torch.exp(x - m).sum(1, keepdim=True)) + m)


def log_softmax_bwd(lp, dlp, dtype=torch.float64):
    return dlp.to(dtype) - torch.exp(lp.to(dtype)) * dlp.to(dtype).sum(1, keepdim=True)


def loss(boxes, boxes_pred, angles, logits, angles_pred, mu, logvar, kl_weight, use_ae, from_logits, dtype=torch.float64):
    """-> dict(losses [4] = (bbox, angle, kl * w, total), angles_pred, d_boxes_pred, d_logits)"""
    O, bd = boxes.shape
    diff = boxes_pred.to(dtype) - boxes.to(dtype)
    lb = diff.abs().double().sum() / (O * bd)
    lp = log_softmax(logits, dtype) if from_logits else angles_pred.to(dtype)
    n = lp.shape[1]
    onehot = torch.zeros(O, n, dtype=dtype)
    onehot[torch.arange(O), angles.long()] = 1
    la = -(lp * onehot).double().sum() / O
    lk = torch.zeros((), dtype=torch.float64)
    if not use_ae:
        m, lv = mu.to(dtype), logvar.to(dtype)
        lk = -0.5 * (1 + lv - m * m - torch.exp(lv)).double().sum() / O * float(kl_weight)
    gb = torch.tensor(1.0, dtype=dtype) / (O * bd)
    return dict(losses=torch.stack([lb, la, lk, lb + la + lk]), angles_pred=lp, d_boxes_pred=torch.sign(diff) * gb,
                d_logits=(torch.exp(lp) - onehot) / O)


def latent_bwd(mu, logvar, eps, dz, kl_weight, use_ae, dtype=torch.float64):
    """dmu = w mu / O + dz; dlogvar = w (exp(lv) - 1) / (2 O) + dz eps exp(lv / 2) / 2 (use_ae: dz, 0)"""
    g = dz.to(dtype)
    if use_ae:
        return g.clone(), torch.zeros_like(g)
    w = torch.tensor(float(kl_weight), dtype=dtype) / dz.shape[0]
    lv = logvar.to(dtype)
    return w * mu.to(dtype) + g, w * 0.5 * (torch.exp(lv) - 1) + g * eps.to(dtype) * 0.5 * torch.exp(0.5 * lv)


# ------------------------------------------------------------------------------------------------ BatchNorm bookkeeping, Adam
def bn_running_update(sums, C, rows, rmean, rvar, momentum, dtype=torch.float64):
    """One application: batch mean and UNBIASED variance (biased at rows == 1, clamped at 0) blended into the running buffers."""
    N = float(rows)
    m = sums[0, :C].double() / N
    v = (sums[1, :C].double() / N - m * m).clamp_min(0.0)
    vu = v * N / (N - 1.0) if rows > 1 else v
    mom = torch.tensor(momentum, dtype=torch.float32).to(dtype)
    return (1 - mom) * rmean[:C].to(dtype) + mom * m.to(dtype), (1 - mom) * rvar[:C].to(dtype) + mom * vu.to(dtype)


def bn_param_grads(gsums, C, dgamma0, dbeta0, dtype=torch.float64):
    """dbeta += sum g, dgamma += sum g * xhat"""
    return dgamma0[:C].to(dtype) + gsums[1, :C].to(dtype), dbeta0[:C].to(dtype) + gsums[0, :C].to(dtype)


def adam(p, g, m, v, step, lr, b1, b2, eps, calls=1, dtype=torch.float64):
    """`calls` updates with the same gradient, starting behind `step` completed ones.  lr, b1, b2, eps: float32 values."""
    p, g, m, v = (t.to(dtype).clone() for t in (p, g, m, v))
    f = lambda x: torch.tensor(x, dtype=torch.float32).to(dtype)
    lr, b1, b2, eps = f(lr), f(b1), f(b2), f(eps)
    for k in range(calls):
        t = step + k + 1
        bc1 = (1.0 - b1.double() ** t).to(dtype)
        bc2 = (1.0 - b2.double() ** t).to(dtype)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - (lr / bc1) * m / (torch.sqrt(v) / torch.sqrt(bc2) + eps)
    return p, m, v, float(bc1), float(bc2)


# ------------------------------------------------------------------------------------------------ Philox-4x32-10, N(0, 1) draw
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr: uint32 [n, 4], key: (k0, k1) -> uint32 [n, 4]; integer arithmetic only"""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & mask, p0 & mask]
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def randn(n, seed, offset, dtype=np.float64):
    """eps[4 q + k], q = counter: key = seed, counter = (q lo, q hi, offset lo, offset hi); words (0, 1) and (2, 3) of a counter
    give two values each by Box-Muller.  The uniforms u1 = (w + 1) 2^-32 in (0, 1], u2 = w 2^-32 and the angle 2 pi u2 are formed
    in float32 as the kernel forms them; log, sqrt, cos and sin are taken in `dtype`."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, offset & 0xFFFFFFFF), np.full_like(q, (offset >> 32) & 0xFFFFFFFF)], 1)
    w = philox4x32_10(ctr.astype(np.uint32), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    k = np.float32(2.3283064365386963e-10)
    out = np.zeros((len(q), 4), dtype=dtype)
    for h in range(2):
        u1 = (w[:, 2 * h].astype(np.float32) + np.float32(1.0)) * k
        u2 = w[:, 2 * h + 1].astype(np.float32) * k
        ang = (np.float32(6.283185307179586) * u2).astype(dtype)
        rad = np.sqrt(dtype(-2.0) * np.log(u1.astype(dtype)))
        out[:, 2 * h] = rad * np.cos(ang)
        out[:, 2 * h + 1] = rad * np.sin(ang)
    return out.reshape(-1)[:n]
