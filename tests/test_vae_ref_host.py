"""tests/vae_ref.py held to something independent of it: autograd of the reference model's expressions (the pooling of oracle/'s
graph conv: index_add over subjects, then objects, divided by the clamped degree), torch.nn.functional losses, nn.BatchNorm1d
buffers, torch.optim.Adam, Philox known-answer vectors - and the ctypes mirrors of the sln_debug_vae_* hooks to sizeof."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import pkg
import vae_ref as V

D64 = torch.float64


def _graph(O, T, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, O, (T,), generator=g)
    o = torch.randint(0, O, (T,), generator=g)
    return g, s, o


def _eval_bn(C_, g):
    return V.Bn(mode=V.BN_EVAL, gamma=torch.rand(C_, generator=g) + 0.5, beta=torch.randn(C_, generator=g) * 0.3,
                rmean=torch.randn(C_, generator=g) * 0.2, rvar=torch.rand(C_, generator=g) + 0.5, eps=1e-5)


def _pool(hs, ho, s, o, O):
    """oracle/vae_ref.py, GraphTripleConv.forward: scatter_add of the subject vectors, then the object vectors, / clamp(count, 1)"""
    pooled = torch.zeros(O, hs.shape[1], dtype=hs.dtype).index_add(0, s, hs).index_add(0, o, ho)
    cnt = torch.zeros(O, dtype=hs.dtype).index_add(0, s, torch.ones(len(s), dtype=hs.dtype)).index_add(0, o, torch.ones(len(o), dtype=hs.dtype))
    return pooled / cnt.clamp(min=1)[:, None]


@pytest.mark.parametrize("O,T,H,D", [(1, 1, 4, 4), (5, 9, 8, 4), (9, 40, 12, 8)])
def test_scatter_forward_and_backward_are_the_pooling_expression_and_its_gradient(O, T, H, D):
    g, s, o = _graph(O, T, 1)
    Cc = 2 * H + D
    A2 = torch.randn(T, Cc + 4, generator=g)
    bn = _eval_bn(Cc, g)
    scale, shift, mean, istd = V.fwd_coef(bn, Cc, D64)
    z = (scale * A2[:, :Cc].double() + shift).requires_grad_(True)
    h = torch.relu(z)
    pooled = _pool(h[:, :H], h[:, H + D:], s, o, O)
    assert torch.allclose(V.scatter_avg_fwd(A2, H, D, bn, s, o, O), pooled, rtol=1e-13, atol=1e-13)
    dM, dP = torch.randn(O, H, generator=g), torch.randn(T, D + 12, generator=g)
    ((pooled * dM.double()).sum() + (h[:, H:H + D] * dP[:, 8:8 + D].double()).sum()).backward()
    g2, gs = V.scatter_avg_bwd(dM, dP, 8, A2, H, D, bn, s, o)
    assert torch.allclose(g2, z.grad, rtol=1e-13, atol=1e-13)
    xhat = (A2[:, :Cc].double() - mean) * istd
    assert torch.allclose(gs, torch.stack([z.grad.sum(0), (z.grad * xhat).sum(0)]), rtol=1e-12, atol=1e-12)
    g2n, _ = V.scatter_avg_bwd(dM, None, 0, A2, H, D, bn, s, o)
    assert torch.equal(g2n[:, H:H + D], torch.zeros(T, D, dtype=D64)) and torch.equal(g2n[:, :H], g2[:, :H])


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("O,T,D", [(1, 3, 4), (17, 50, 8)])
def test_gather_backward_is_the_gradient_of_the_triple_concat(O, T, D, masked):
    g, s, o = _graph(O, T, 2)
    xprev = torch.randn(O, D + 4, generator=g)
    bn = _eval_bn(D, g)
    scale, shift, _, _ = V.fwd_coef(bn, D, D64)
    z = (scale * xprev[:, :D].double() + shift).requires_grad_(True)
    obj = torch.relu(z) if masked else z
    dG, add1 = torch.randn(T, 3 * D + 4, generator=g), torch.randn(O, D + 8, generator=g)
    cur = torch.cat([obj[s], torch.zeros(T, D, dtype=D64), obj[o]], 1)          # graph conv input [obj[s] | pred | obj[o]]
    ((cur * dG[:, :3 * D].double()).sum() + (obj * add1[:, :D].double()).sum()).backward()
    d, _ = V.gather_bwd(dG, D, s, o, O, add1, xprev, bn, masked)
    assert torch.allclose(d, z.grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("rows,cols", [(1, 1), (33, 65)])
def test_mask_and_statistics_are_batchnorm_relu_autograd(rows, cols):
    g = torch.Generator().manual_seed(3)
    xprev = torch.randn(rows, cols, generator=g).double()
    bnm = torch.nn.BatchNorm1d(cols, eps=1e-5).double().train()
    with torch.no_grad():
        bnm.weight.copy_(torch.rand(cols, generator=g) + 0.5); bnm.bias.copy_(torch.randn(cols, generator=g) * 0.3)
    d1, d2 = torch.randn(rows, cols, generator=g).double(), torch.randn(rows, cols, generator=g).double()
    if rows == 1:          # nn.BatchNorm1d refuses one row in train mode: the same statistics through F.batch_norm's formula
        z = ((xprev - xprev.mean(0)) / torch.sqrt(xprev.var(0, unbiased=False) + 1e-5) * bnm.weight + bnm.bias)
    else:
        z = bnm(xprev)
    z.retain_grad()
    (torch.relu(z) * (d1 + d2)).sum().backward()
    bn = V.Bn(mode=V.BN_TRAIN, gamma=bnm.weight.detach().float(), beta=bnm.bias.detach().float(), sums=V.sums_of(xprev), n_rows=float(rows), eps=1e-5)
    bn.gamma, bn.beta = bnm.weight.detach(), bnm.bias.detach()
    d, gs = V.mask_gstats(d1, d2, xprev, bn, rows, cols)
    assert torch.allclose(d, z.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(gs[0], bnm.bias.grad, rtol=1e-10, atol=1e-10) and torch.allclose(gs[1], bnm.weight.grad, rtol=1e-9, atol=1e-9)
    dg, db = V.bn_param_grads(gs, cols, torch.ones(cols), torch.full((cols,), 2.0))
    assert torch.allclose(dg, 1 + bnm.weight.grad, rtol=1e-9, atol=1e-9) and torch.allclose(db, 2 + bnm.bias.grad, rtol=1e-9, atol=1e-9)
    assert torch.allclose(V.bn_relu_apply(xprev, 0, cols, bn), torch.relu(z).detach(), rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("box_dim,n_attr", [(4, 0), (6, 5)])
def test_embedding_assembly_box_linear_and_their_gradients(box_dim, n_attr):
    g = torch.Generator().manual_seed(4)
    O, n_obj, n_box, n_angle = 19, 7, 9, 3
    objs, attrs, angles = (torch.randint(0, k, (O,), generator=g) for k in (6, 4, 5))
    boxes = torch.rand(O, box_dim, generator=g)
    E = [torch.randn(6, n_obj, generator=g).double().requires_grad_(True), torch.randn(4, max(n_attr, 1), generator=g).double().requires_grad_(True),
         torch.randn(5, n_angle, generator=g).double().requires_grad_(True)]
    lin = torch.nn.Linear(box_dim, n_box).double()
    parts = [F.embedding(objs, E[0])] + ([F.embedding(attrs, E[1])] if n_attr else []) + [lin(boxes.double()), F.embedding(angles, E[2])]
    x0 = torch.cat(parts, 1)
    ref = V.enc_assemble(objs, attrs, angles, boxes, E[0].detach(), E[1].detach() if n_attr else None, E[2].detach(), lin.weight.detach(), lin.bias.detach())
    assert torch.allclose(ref, x0, rtol=1e-13, atol=1e-13)
    dx0 = torch.randn(O, x0.shape[1], generator=g).double()
    (x0 * dx0).sum().backward()
    pre = torch.full((6, n_obj), 0.5)
    assert torch.allclose(V.embed_bwd(objs, dx0, 0, n_obj, pre), 0.5 + E[0].grad, rtol=1e-13, atol=1e-13)
    c = n_obj + n_attr
    dwb, dbb = V.box_linear_bwd(dx0[:, c:c + n_box], boxes, torch.ones(n_box, box_dim), torch.ones(n_box))
    assert torch.allclose(dwb, 1 + lin.weight.grad, rtol=1e-12, atol=1e-12) and torch.allclose(dbb, 1 + lin.bias.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(V.embed_bwd(angles, dx0, c + n_box, n_angle, torch.zeros(5, n_angle)), E[2].grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("O,n_angle", [(1, 1), (7, 24), (33, 9)])
def test_loss_terms_and_gradients_are_the_functional_losses(O, n_angle):
    g = torch.Generator().manual_seed(5)
    bd, nz, w = 6, 8, 0.37
    boxes, bp = torch.rand(O, bd, generator=g), torch.rand(O, bd, generator=g).double().requires_grad_(True)
    logits = (torch.randn(O, n_angle, generator=g) * 3).double().requires_grad_(True)
    angles = torch.randint(0, n_angle, (O,), generator=g)
    mu, lv = torch.randn(O, nz, generator=g).double().requires_grad_(True), (torch.randn(O, nz, generator=g) * 0.5).double().requires_grad_(True)
    eps = torch.randn(O, nz, generator=g)
    lp = F.log_softmax(logits, 1)
    lb, la = F.l1_loss(bp, boxes.double()), F.nll_loss(lp, angles)
    lk = -0.5 * torch.sum(1 + lv - mu.pow(2) - lv.exp()) / O * w          # utils.py:12-33 of the reference model
    z = eps.double() * torch.exp(0.5 * lv) + mu
    dz = torch.randn(O, nz, generator=g).double()
    (lb + la + lk + (z * dz).sum()).backward()
    r = V.loss(boxes, bp.detach(), angles, logits.detach(), None, mu.detach(), lv.detach(), w, 0, 1)
    assert torch.allclose(r["losses"], torch.stack([lb, la, lk, lb + la + lk]).detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(r["angles_pred"], lp.detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(r["d_boxes_pred"], bp.grad, rtol=1e-13, atol=0) and torch.allclose(r["d_logits"], logits.grad, rtol=1e-12, atol=1e-15)
    r2 = V.loss(boxes, bp.detach(), angles, None, lp.detach(), None, None, w, 1, 0)
    assert float(r2["losses"][2]) == 0.0 and torch.allclose(r2["losses"][3], (lb + la).detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(V.reparam(mu.detach(), lv.detach(), eps), z.detach(), rtol=1e-14, atol=1e-14)
    dmu, dlv = V.latent_bwd(mu.detach(), lv.detach(), eps, dz, w, 0)
    assert torch.allclose(dmu, mu.grad, rtol=1e-12, atol=1e-14) and torch.allclose(dlv, lv.grad, rtol=1e-12, atol=1e-14)
    dlp = torch.randn(O, n_angle, generator=g).double()
    x = logits.detach().clone().requires_grad_(True)
    (F.log_softmax(x, 1) * dlp).sum().backward()
    assert torch.allclose(V.log_softmax_bwd(lp.detach(), dlp), x.grad, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("rows", [2, 12])
def test_running_statistics_are_batchnorm1d_buffers_after_one_and_two_applications(rows):
    g = torch.Generator().manual_seed(6)
    Cc = 5
    bnm = torch.nn.BatchNorm1d(Cc, momentum=0.1).double().train()
    rm, rv = torch.zeros(Cc, dtype=D64), torch.ones(Cc, dtype=D64)
    for k in range(2):
        x = torch.randn(rows, Cc, generator=g).double() * (k + 1) + k
        bnm(x)
        rm, rv = V.bn_running_update(V.sums_of(x), Cc, rows, rm, rv, 0.1)
        # (the momentum is the float32 0.1 the kernel is handed: 1.5e-9 from the module's double)
        assert torch.allclose(rm, bnm.running_mean, rtol=1e-8, atol=1e-8) and torch.allclose(rv, bnm.running_var, rtol=1e-8, atol=1e-8)
    assert int(bnm.num_batches_tracked) == 2
    one = torch.tensor([[3.0], [9.0]], dtype=D64)           # rows == 1: sum 3, sum of squares 9 - no Bessel factor, variance 0
    m1, v1 = V.bn_running_update(one, 1, 1, torch.zeros(1), torch.ones(1), 0.5)
    assert float(m1) == 1.5 and float(v1) == 0.5
    neg = torch.tensor([[4.0], [7.999999]], dtype=D64)      # E[x^2] - mean^2 slightly negative: clamped
    assert float(V.bn_running_update(neg, 1, 2, torch.zeros(1), torch.zeros(1), 0.5)[1]) == 0.0


def test_adam_is_torch_optim_adam_over_three_steps():
    g = torch.Generator().manual_seed(7)
    n = 37
    f32 = lambda x: float(np.float32(x))
    p0, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    par = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([par], lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8))
    for _ in range(3):
        par.grad = grad.double().clone()
        opt.step()
    p, m, v, bc1, bc2 = V.adam(p0, grad, torch.zeros(n), torch.zeros(n), 0, 1e-3, 0.9, 0.999, 1e-8, calls=3)
    st = opt.state[par]
    assert torch.allclose(p, par.detach(), rtol=1e-12, atol=1e-14)
    assert torch.allclose(m, st["exp_avg"], rtol=1e-13, atol=0) and torch.allclose(v, st["exp_avg_sq"], rtol=1e-13, atol=0)
    assert abs(bc1 - (1 - f32(0.9) ** 3)) < 1e-15 and abs(bc2 - (1 - f32(0.999) ** 3)) < 1e-15


def test_philox_known_answers():
    """Philox-4x32-10 of Salmon et al.: the Random123 known-answer vectors, recomputed from the kernel's round function"""
    got = V.philox4x32_10(np.zeros((1, 4), dtype=np.uint32), (0, 0))
    assert [hex(int(x)) for x in got[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    got = V.philox4x32_10(np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], dtype=np.uint32), (0xa4093822, 0x299f31d0))
    assert [hex(int(x)) for x in got[0]] == ["0xd16cfe09", "0x94fdcceb", "0x5001e420", "0x24126ea1"]


def test_randn_reference_is_a_standard_normal_and_follows_its_counters():
    a = V.randn(40001, 0x1234567800000042, (1 << 32) + 5)
    assert abs(a.mean()) < 0.02 and abs(a.std() - 1) < 0.02 and np.isfinite(a).all()
    assert np.array_equal(V.randn(5, 7, 9), V.randn(1025, 7, 9)[:5])
    assert not np.array_equal(V.randn(8, 7, 9), V.randn(8, 7, 10)) and not np.array_equal(V.randn(8, 7, 9), V.randn(8, 7 + (1 << 32), 9))


def test_csr_reference_rows_are_ascending_and_complete():
    tri = torch.tensor([[0, 1, 2], [2, 0, 2], [1, 5, 0], [9, 0, 0]])          # predicate 5 and subject 9 are out of range
    r = V.csr(tri, 3, 3)
    assert r["err"] == 1 and r["rows"] == [[0, 2, 3, 6, 7], [], [1, 4, 5]] and r["deg"].tolist() == [5, 0, 3] and r["rowptr"].tolist() == [0, 5, 5, 8]
    assert r["s"].tolist() == [0, 2, 0, 0] and r["p"].tolist() == [1, 0, 0, 0]


def test_ctypes_mirrors_of_the_vae_hooks_have_the_headers_sizes():
    L = pkg("_lib")
    names = ("SlnDbgCsr", "SlnDbgEdge", "SlnDbgLoss", "SlnDbgBnEntry", "SlnDbgTranspose", "SlnDbgOpt", "SlnDbgEmbed")
    out = (C.c_int * len(names))()
    assert L.lib().sln_debug_vae_sizes(out, len(names)) == len(names)
    assert list(out) == [C.sizeof(getattr(L, n)) for n in names]
    assert C.sizeof(L.SlnDbgEdge) == C.sizeof(L.SlnDbgCsr) + C.sizeof(L.SlnDbgBn) + 5 * 8 + 12 * 4
