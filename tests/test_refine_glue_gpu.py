"""The glue launches of a refinement iteration at operand level (csrc/placement.hip): the head kernels over the concatenated rows of
several rooms (sln_refine_head_*_rooms), the head inside the two placement launches (SlnPlacementRoom::boxes_pred, with the device
counter that selects the iteration's noise row), and the update launches (sln_refine_sgd_rooms, sln_refine_sgd).

References: oracle/refine_ref.py (softargmax, fix_grad, quad_grad) in fp64 with the tolerance rule of test_refine_loss_family_gpu.py
(4 x the fp32 evaluation's distance from fp64 + 2e-6 x max|ref|); the stand-alone kernels for the bits of the head-in-LDS path;
p - step * g in fp64 with one rounding of the product and one of the difference for the updates.  The refusals of the update launches,
which return before anything is launched, are in test_refine_loss_cases_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import SENT, _lib, _sync
from oracle import refine_ref

import test_place_views_gpu as PV
from test_refine_loss_family_gpu import _bits, _close, _full, _tail_ok

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ROOM_ROWS = [1, 2, 13, 13, 13, 13, 13, 2]      # a room of the frozen row alone, of 2 and of 13 rows; 70 rows cross the 64-thread block
N_ANGLE, BETA = 24, 2.0


# ------------------------------------------------------------------------------------------- the head over the rows of several rooms
def _head_case(big, seed):
    rows = ROOM_ROWS
    N, R = sum(rows), len(rows)
    assert N == 70 and N > 64
    g = torch.Generator().manual_seed(seed)
    room_of_row = torch.tensor([r for r, n in enumerate(rows) for _ in range(n)], dtype=torch.int32)
    last_row = torch.tensor(np.cumsum(rows) - 1, dtype=torch.int32)
    bp = torch.randn(N, 6, generator=g)
    ap = torch.randn(N, N_ANGLE, generator=g) * 3
    if big:                                                      # beta * 40 = 80: only the max shift keeps exp away from the end of fp32
        ap = torch.where(torch.rand(N, N_ANGLE, generator=g) < 0.5, torch.full_like(ap, 40.0), torch.full_like(ap, -40.0))
        ap[5] = 40.0; ap[6] = -40.0; ap[7, 1:] = -40.0; ap[7, 0] = 40.0
        ap[8, ::2] = 50.0; ap[8, 1::2] = -50.0; ap[9] = 50.0     # exp(100) is inf in fp32, exp(80) = 5.5e34 only nearly
    noise = torch.randn(N, generator=g)
    box_last, angle_last = torch.rand(R, 6, generator=g), torch.rand(R, generator=g) * 23
    gb, gi = torch.randn(N, 6, generator=g), torch.randn(N, generator=g)
    frozen = torch.zeros(N, dtype=torch.bool)
    frozen[last_row.long()] = True
    return dict(N=N, R=R, room_of_row=room_of_row, last_row=last_row, bp=bp, ap=ap, noise=noise, box_last=box_last, angle_last=angle_last, gb=gb, gi=gi,
                frozen=frozen)


def _head_reference(p, with_noise, dtype):
    """-> (idx [N], grad_boxes_pred [N, 6], grad_angles_pred [N, 24]): test_render_refine.py:296-306 with both gradient hooks, frozen rows cut"""
    ap = p["ap"].to(dtype).requires_grad_(True)
    idx = refine_ref.softargmax(ap, BETA)
    if with_noise:
        idx = idx + p["noise"].to(dtype) / 10.0
    idx.register_hook(refine_ref.quad_grad)
    live = ~p["frozen"]
    (idx * p["gi"].to(dtype))[live].sum().backward()
    full = torch.where(p["frozen"], p["angle_last"].to(dtype)[p["room_of_row"].long()], idx.detach())
    gbp = refine_ref.fix_grad(p["gb"].to(dtype))
    gbp[p["frozen"]] = 0.0
    return full, gbp, ap.grad


@pytest.mark.parametrize("ld_gb", [6, 8])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("big", [False, True])
def test_head_kernels_over_the_rows_of_several_rooms(big, with_noise, ld_gb):
    L = _lib()
    lib, P = L.lib(), L.ptr
    p = _head_case(big, seed=11 + int(big))
    N = p["N"]
    dev = {k: v.cuda() for k, v in p.items() if torch.is_tensor(v)}
    noise = dev["noise"] if with_noise else None
    route = "head rooms: rows %s, logits %s, noise %s, ld_gb %d" % (ROOM_ROWS, "+-40 and +-50" if big else "randn * 3", "given" if with_noise else "NULL", ld_gb)
    boxes_full, idx = _full(6 * N), _full(N)
    L.check(lib.sln_refine_head_forward_rooms(N, N_ANGLE, P(dev["room_of_row"]), P(dev["last_row"]), P(dev["bp"]), P(dev["ap"]), P(noise),
                                              P(dev["box_last"]), P(dev["angle_last"]), BETA, P(boxes_full), P(idx), L.current_stream_ptr()),
            "sln_refine_head_forward_rooms")
    _sync("sln_refine_head_forward_rooms")
    _tail_ok(boxes_full, 6 * N, "boxes_full"); _tail_ok(idx, N, "idx")
    r64, r32 = _head_reference(p, with_noise, F64), _head_reference(p, with_noise, F32)
    want_boxes = torch.where(p["frozen"][:, None], p["box_last"][p["room_of_row"].long()], p["bp"])
    assert _bits(boxes_full[:6 * N].view(N, 6).cpu(), want_boxes), "boxes_full is a copy: boxes_pred, the room's box_last in its frozen row"
    got_idx = idx[:N].cpu()
    assert _bits(got_idx[p["frozen"]], p["angle_last"]), "the frozen rows' angle is angle_last, bit for bit"
    assert bool(torch.isfinite(got_idx).all())
    lines = [_close(got_idx, r64[0], r32[0], "idx", route)]
    gbp, gap = _full(ld_gb * N), _full(N_ANGLE * N)
    L.check(lib.sln_refine_head_backward_rooms(N, N_ANGLE, P(dev["room_of_row"]), P(dev["last_row"]), P(dev["ap"]), P(dev["gb"]), P(dev["gi"]), BETA,
                                               P(gbp), ld_gb, P(gap), L.current_stream_ptr()), "sln_refine_head_backward_rooms")
    _sync("sln_refine_head_backward_rooms")
    _tail_ok(gbp, ld_gb * N, "grad_boxes_pred"); _tail_ok(gap, N_ANGLE * N, "grad_angles_pred")
    got_b, got_a = gbp[:ld_gb * N].view(N, ld_gb).cpu(), gap[:N_ANGLE * N].view(N, N_ANGLE).cpu()
    assert float(got_b[:, 6:].abs().max() if ld_gb > 6 else 0.0) == 0.0, "the padding columns are zeros"
    assert float(got_b[p["frozen"]].abs().max()) == 0.0 and float(got_a[p["frozen"]].abs().max()) == 0.0, "frozen rows get exact zeros"
    lines.append(_close(got_b[:, :6], r64[1], r32[1], "grad_boxes_pred", route))
    lines.append(_close(got_a, r64[2], r32[2], "grad_angles_pred", route))
    assert float(r64[2].abs().max()) > 0
    print("\n".join(lines) + "\nroute: " + route)


# ------------------------------------------------------------------------------------------- the head inside the placement launches
class HeadBufs(PV.Bufs):
    """PV.Bufs (the two rooms of test_place_views_gpu.py, one view) with the decoder's outputs, a [3, stride] noise table and the frozen
    rows; ``head=True`` puts them into the rooms' table (the head then runs inside the placement launches), otherwise the table stays as
    it is and ``head_forward`` / ``head_backward`` are the stand-alone launches"""
    LD_GB = 8

    def __init__(self, head):
        super().__init__(1)
        L = pkg("_lib")
        N, R = self.N, self.R
        g = torch.Generator().manual_seed(5)
        self.boxes_pred = self.boxes.clone()
        self.angles_pred = (torch.randn(N, N_ANGLE, generator=g) * 3).cuda()
        self.noise_stride = N + 3
        self.noise = torch.randn(3, self.noise_stride, generator=g).cuda()
        last = [self.row0[r] + self.rows[r] - 1 for r in range(R)]
        self.box_last = self.boxes[last].clone().contiguous()
        self.angle_last = self.idx[last].clone().contiguous()
        self.room_of_row = torch.tensor([r for r in range(R) for _ in range(self.rows[r])], dtype=torch.int32).cuda()
        self.last_row = torch.tensor(last, dtype=torch.int32).cuda()
        self.counter = torch.zeros(1 + PV.TAIL, dtype=torch.int32, device="cuda")
        self._gbp, self._gap = _full(self.LD_GB * N), _full(N_ANGLE * N)
        self.boxes.fill_(SENT); self.idx.fill_(SENT)             # the forward derives and stores them
        if head:
            tab = (L.SlnPlacementRoom * R).from_buffer_copy(bytes(self.tab.cpu().numpy().tobytes()))
            for r in range(R):
                e, a = tab[r], self.row0[r]
                assert e.P.n == self.rows[r] <= 128
                e.boxes_pred, e.angles_pred = self.boxes_pred.data_ptr() + 24 * a, self.angles_pred.data_ptr() + 4 * N_ANGLE * a
                e.noise, e.noise_step, e.noise_stride = self.noise.data_ptr() + 4 * a, self.counter.data_ptr(), self.noise_stride
                e.box_last, e.angle_last = self.box_last.data_ptr() + 24 * r, self.angle_last.data_ptr() + 4 * r
                e.grad_boxes_pred, e.grad_angles_pred = self._gbp.data_ptr() + 4 * self.LD_GB * a, self._gap.data_ptr() + 4 * N_ANGLE * a
                e.n_angle, e.ld_gb, e.beta = N_ANGLE, self.LD_GB, BETA
            self.tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()

    def head_forward(self, step):
        L = pkg("_lib")
        P = L.ptr
        L.check(L.lib().sln_refine_head_forward_rooms(self.N, N_ANGLE, P(self.room_of_row), P(self.last_row), P(self.boxes_pred), P(self.angles_pred),
                                                      P(self.noise[step]), P(self.box_last), P(self.angle_last), BETA, P(self.boxes), P(self.idx),
                                                      L.current_stream_ptr()), "sln_refine_head_forward_rooms")

    def head_backward(self):
        L = pkg("_lib")
        P = L.ptr
        L.check(L.lib().sln_refine_head_backward_rooms(self.N, N_ANGLE, P(self.room_of_row), P(self.last_row), P(self.angles_pred), P(self.g_boxes),
                                                       P(self.g_idx), BETA, P(self._gbp), self.LD_GB, P(self._gap), L.current_stream_ptr()),
                "sln_refine_head_backward_rooms")

    def snapshot(self):
        out = dict(self.outputs(), boxes=self.boxes, idx=self.idx, grad_boxes_pred=self._gbp, grad_angles_pred=self._gap)
        return {k: v.clone() for k, v in out.items()}


def test_head_inside_the_placement_launches_equals_the_stand_alone_steps():
    """With the head fields set, forward + backward of sln_place_*_rooms give the bits of: stand-alone head forward on the noise row the
    counter names, the same placement launches without head fields, stand-alone head backward.  The counter starts at 0, is 1 after the first
    pair and 2 after the second, and the second forward reads noise row 1."""
    alone, fused = HeadBufs(head=False), HeadBufs(head=True)
    assert max(fused.rows) <= 128
    seen = []
    for step in (0, 1):
        alone.head_forward(step)
        _sync("stand-alone head forward, step %d" % step)
        alone.single()
        _sync("placement without head fields, step %d" % step)
        alone.head_backward()
        _sync("stand-alone head backward, step %d" % step)
        want = alone.snapshot()
        fused.single()
        _sync("head inside the placement launches, step %d" % step)
        got = fused.snapshot()
        alone.check_sentinels(); fused.check_sentinels()
        for name in want:
            assert _bits(got[name], want[name]), "step %d: %s differs from the stand-alone launches in %d elements" % (
                step, name, int((got[name] != want[name]).sum()))
        for buf, n in ((fused._gbp, fused.LD_GB * fused.N), (fused._gap, N_ANGLE * fused.N)):
            _tail_ok(buf, n, "head gradients"); assert not bool((buf[:n] == SENT).any())
        assert not bool((fused.boxes == SENT).any()) and not bool((fused.idx == SENT).any()), "the forward stores the boxes / angles it derived"
        assert float(fused._gbp[:fused.LD_GB * fused.N].view(-1, fused.LD_GB)[:, 6:].abs().max()) == 0.0
        cnt = fused.counter.cpu()
        assert int(cnt[0]) == step + 1 and not bool(cnt[1:].any()), "the counter after %d pair(s): %s" % (step + 1, cnt[:2].tolist())
        seen.append(got)
    assert int(alone.counter.cpu()[0]) == 0, "without head fields nothing advances a counter"
    assert not _bits(seen[0]["idx"], seen[1]["idx"]) and not _bits(seen[0]["faces"], seen[1]["faces"]), "the second pair read another noise row"
    print("head in LDS: faces, sizes, size loss, boxes, idx and both head gradients bit-equal to the stand-alone launches over 2 steps; counter 0 -> 1 -> 2")


# ------------------------------------------------------------------------------------------------------------------ the update launches
def _update_bound(got, p, g, step, what):
    """|got - (p - step * g)| <= 2^-23 (|p| + |step * g|): one rounding of the product and one of the difference, contracted or not"""
    step = float(np.float32(step))
    prod = step * g.double()
    ref = p.double() - prod
    err = (got.double() - ref).abs()
    tol = 2.0 ** -23 * (p.double().abs() + prod.abs())
    bad = (err > tol).nonzero()
    assert bad.numel() == 0, "%s: %d elements off, first at %s: err %.3e bound %.3e" % (
        what, bad.shape[0], tuple(int(v) for v in bad[0]), float(err[tuple(bad[0])]), float(tol[tuple(bad[0])]))
    return float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0


RANGES = [(8, 40), (100, 2048), (2400, 0), (3000, 1000)]       # three ranges with gaps between them and an empty one; 2048 / 4 = 2 blocks
STRIDE = 4096


@pytest.mark.parametrize("nz", [5, 700])                       # below every len / 4 of the stepped ranges' largest (512), and above: either sizes the grid
@pytest.mark.parametrize("R", [1, 3])
def test_update_of_several_parameter_copies(R, nz):
    L = _lib()
    lib, P = L.lib(), L.ptr
    g_ = torch.Generator().manual_seed(100 * R + nz)
    n = R * STRIDE
    p0, g0 = torch.randn(n + PV.TAIL, generator=g_), torch.randn(n + PV.TAIL, generator=g_)
    z0, gz = torch.randn(nz + PV.TAIL, generator=g_), torch.randn(nz + PV.TAIL, generator=g_)
    p, g, z, gzd = p0.cuda(), g0.cuda(), z0.cuda(), gz.cuda()
    off, ln = [(C.c_int64 * len(RANGES))(*[r[k] for r in RANGES]) for k in (0, 1)]
    step, step_z = 0.011, 0.00022
    assert all(o % 4 == 0 and l % 4 == 0 and o + l <= STRIDE for o, l in RANGES) and STRIDE % 4 == 0
    assert min(l // 4 for _, l in RANGES if l) > 5 and max(l // 4 for _, l in RANGES) < 700
    L.check(lib.sln_refine_sgd_rooms(P(p), P(g), R, STRIDE, off, ln, len(RANGES), step, P(z), P(gzd), nz, step_z, L.current_stream_ptr()),
            "sln_refine_sgd_rooms")
    _sync("sln_refine_sgd_rooms")
    p1, g1, z1 = p.cpu(), g.cpu(), z.cpu()
    inside = torch.zeros(n + PV.TAIL, dtype=torch.bool)
    for r in range(R):
        for o, l in RANGES:
            inside[r * STRIDE + o:r * STRIDE + o + l] = True
    assert int(inside.sum()) == R * sum(l for _, l in RANGES)
    worst = _update_bound(p1[inside], p0[inside], g0[inside], step, "parameters")
    assert float(g1[inside].abs().max()) == 0.0, "stepped gradients are exactly 0"
    assert _bits(p1[~inside], p0[~inside]) and _bits(g1[~inside], g0[~inside]), "the gaps and everything behind R * stride keep their bits"
    worst_z = _update_bound(z1[:nz], z0[:nz], gz[:nz], step_z, "z (stepped once, not R = %d times)" % R)
    assert _bits(z1[nz:], z0[nz:]) and bool((z1[:nz] != z0[:nz]).any())
    assert torch.equal(gzd.cpu(), gz)
    print("sln_refine_sgd_rooms R %d nz %d: worst err / bound %.2f (parameters) %.2f (z)" % (R, nz, worst, worst_z))


@pytest.mark.parametrize("nz", [0, 300])
@pytest.mark.parametrize("n", [3, 1031])
def test_update_of_one_parameter_copy(n, nz):
    """sln_refine_sgd at sizes that are no multiple of 4 (the float4 body and the scalar tail), with no z and with more z than n / 4"""
    L = _lib()
    lib, P = L.lib(), L.ptr
    g_ = torch.Generator().manual_seed(7 * n + nz)
    p0, g0 = torch.randn(n + PV.TAIL, generator=g_), torch.randn(n + PV.TAIL, generator=g_)
    z0, gz = torch.randn(nz + PV.TAIL, generator=g_), torch.randn(nz + PV.TAIL, generator=g_)
    p, g, z, gzd = p0.cuda(), g0.cuda(), z0.cuda(), gz.cuda()
    assert nz == 0 or nz > n // 4 + n % 4
    L.check(lib.sln_refine_sgd(P(p), P(g), n, 0.011, P(z) if nz else None, P(gzd) if nz else None, nz, 0.00022, L.current_stream_ptr()), "sln_refine_sgd")
    _sync("sln_refine_sgd")
    p1, g1, z1 = p.cpu(), g.cpu(), z.cpu()
    worst = _update_bound(p1[:n], p0[:n], g0[:n], 0.011, "parameters")
    assert float(g1[:n].abs().max()) == 0.0
    assert _bits(p1[n:], p0[n:]) and _bits(g1[n:], g0[n:]), "nothing behind n is touched"
    worst_z = _update_bound(z1[:nz], z0[:nz], gz[:nz], 0.00022, "z")
    assert _bits(z1[nz:], z0[nz:])
    print("sln_refine_sgd n %d nz %d: worst err / bound %.2f (parameters) %.2f (z)" % (n, nz, worst, worst_z))
