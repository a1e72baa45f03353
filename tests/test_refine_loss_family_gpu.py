"""csrc/refine_loss.hip at operand level, every element, per route (tests/refine_loss_cases.py: sign-safe operands at the smallest
geometries at which each pooling / backward route and each shape edge exists; test_refine_loss_cases_host.py holds the operands to the
margins that make the comparison of every element legitimate).

The reference is oracle/refine_ref.py (host.refine.refinement_loss_masked under a mask) in fp64 on the CPU.  Tolerance of a tensor:
4 * yardstick + 2e-6 * max|ref|, the yardstick being max |fp32 - fp64| of the same reference function (the factor this project gives its
fp32 kernels over the fp32 reference, and gpu_util's floor).  Every case prints err / bound / yardstick and the route its launches take."""
import ctypes as C
import functools

import pytest
import torch

from conftest import pkg
from gpu_util import SENT, _assert_close, _lib, _sync

import refine_loss_cases as RC

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TAIL = 64
WS_FILL, WS_TAIL = 0xA5, 256
E_UNSUPPORTED = -2


def _close(got, ref64, ref32, what, route):
    """|got - fp64| <= 4 * max|fp32 - fp64| + 2e-6 * max|fp64| over EVERY element; -> 'what: err bound yardstick'"""
    ref64, ref32 = ref64.detach().double(), ref32.detach()
    yard = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    e, tol = _assert_close(got.detach().cpu(), ref64, 2e-6, 4.0 * yard / max(1.0, scale), what, route)
    return "%s err %.3e bound %.3e fp32-yardstick %.3e" % (what, e, tol, yard)


def _full(n, dtype=torch.float32):
    """n elements of SENT and TAIL more behind them"""
    return torch.full((n + TAIL,), SENT, dtype=dtype, device="cuda")


def _tail_ok(buf, n, what):
    assert bool((buf[n:] == SENT).all()), "%s: a write behind the output" % what


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _copy(desc):
    return type(desc).from_buffer_copy(desc)


class Setup:
    """The device side of a case: the product's own target preparation (RefineLoss: pooled target depth, labels, counts, the mask call), the
    iterate (with the case's extra channels behind dep0 + n_dep), a workspace with a guarded tail."""

    def __init__(self, name):
        self.L = _lib()
        self.lib = self.L.lib()
        R = pkg("host.refine")
        self.c, self.ops = RC.BY_NAME[name], RC.operands(name)
        c = self.c
        self.B, self.S, self.P, self.ns, self.nd = c["B"], c["S"], c["sizes"][-1], len(c["sizes"]), c["C"] - 41
        self.route = "%s: %s" % (name, RC.route(c))
        valid = self.ops["valid"]
        self.valid = valid.cuda() if valid is not None else None
        self.rl = R.RefineLoss(self.ops["target"].cuda(), sizes=c["sizes"], per_room=c["per_room"], valid=self.valid)
        _sync("RefineLoss(%s)" % name)
        self.C = c["C"] + c["extra_channels"]
        g = torch.Generator().manual_seed(77)
        extra = torch.randn(self.B, c["extra_channels"], self.S, self.S, generator=g)
        self.image = torch.cat([self.ops["image"], extra], 1).contiguous().cuda()
        self.desc = _copy(self.rl.desc)
        self.desc.channels = self.C
        assert self.desc.n_dep == self.nd and self.desc.dep0 + self.nd == c["C"]
        assert (self.desc.stage1_stride, self.desc.pooled_size, self.desc.max_col_entries) == RC.host_tables(c["S"], c["sizes"])[:3]
        self.ws_bytes = int(self.lib.sln_refine_loss_workspace_bytes(self.B, self.S, self.P, self.ns, 40, self.nd))
        self.ws = torch.full((self.ws_bytes + WS_TAIL,), WS_FILL, dtype=torch.uint8, device="cuda")
        self.n_pooled = self.B * self.ns * (40 + self.nd) * self.P * self.P
        self.n_loss = 3 * self.B if c["per_room"] else 3

    def sp(self):
        return self.L.current_stream_ptr()

    def ws_ok(self, what):
        assert bool((self.ws[self.ws_bytes:] == WS_FILL).all()), "%s: a write behind the workspace" % what

    def pool(self, desc, image, null_fill, what):
        out = _full(self.n_pooled)
        self.L.check(self.lib.sln_refine_pool(desc, self.L.ptr(image), null_fill, self.L.ptr(self.ws), self.L.ptr(out), self.sp()), what)
        _sync(what)
        _tail_ok(out, self.n_pooled, what); self.ws_ok(what)
        return out[:self.n_pooled].view(self.B, self.ns, 40 + self.nd, self.P, self.P)

    def forward(self, desc, image, what):
        out = _full(self.n_loss)
        rl = self.rl
        self.L.check(self.lib.sln_refine_loss_forward(desc, self.L.ptr(image), self.L.ptr(rl.target_depth), self.L.ptr(rl.labels), self.L.ptr(rl.inv_count),
                                                      self.L.ptr(self.ws), self.L.ptr(out), self.sp()), what)
        _sync(what)
        _tail_ok(out, self.n_loss, what); self.ws_ok(what)
        return out[:self.n_loss].view(-1, 3) if self.c["per_room"] else out[:3]

    def backward(self, desc, scale, what, image_shape=None):
        shape = tuple(self.image.shape) if image_shape is None else image_shape
        n = 1
        for v in shape:
            n *= v
        out = _full(n)
        self.L.check(self.lib.sln_refine_loss_backward(desc, self.L.ptr(self.ws), self.L.ptr(scale), self.L.ptr(out), self.sp()), what)
        _sync(what)
        _tail_ok(out, n, what); self.ws_ok(what)
        return out[:n].view(shape)


@functools.lru_cache(maxsize=None)
def setup(name):
    return Setup(name)


# ------------------------------------------------------------------------------------------------------------------ 1. the pooling
@pytest.mark.parametrize("null_fill", [0, 1])
@pytest.mark.parametrize("name", RC.NAMES)
def test_pool_against_fp64(name, null_fill):
    """sln_refine_pool of the iterate (null_fill 1: with the last depth plane filled where no class has depth) against fp64 psp_pool:
    all B * n_scales * (C - 1) * P * P elements, nothing behind them written"""
    s = setup(name)
    got = s.pool(s.desc, s.image, null_fill, "sln_refine_pool(%s, %d)" % (name, null_fill))
    image = s.ops["image"]
    ref64, ref32 = RC.pooled(image, s.c["sizes"], null_fill, F64), RC.pooled(image, s.c["sizes"], null_fill, F32)
    assert ref64.shape == got.shape
    if null_fill:
        assert float((ref64 - RC.pooled(image, s.c["sizes"], 0, F64))[:, :, -1].abs().max()) > 0.5, "the fill shows in the last plane"
    print(_close(got, ref64, ref32, "pooled[null_fill %d]" % null_fill, s.route) + "; route: " + s.route)


# ------------------------------------------------------------------------- 2. pool_kernel against pool_lds_kernel, bit for bit
@pytest.mark.parametrize("null_fill", [0, 1])
@pytest.mark.parametrize("name", ["s40-b3-rooms", "s40-ndep11-b3", "generic-b3-batch", "tail-b3-batch"])
def test_plain_pooling_kernel_gives_the_bits_of_the_lds_kernel(name, null_fill):
    """The stage-1 tables of an LDS-route case copied into rows of stride 104: the stride is only a row length, the descriptor stays legal,
    and launch_pool takes pool_kernel (stage1_stride > 96).  'Same expressions, same order: the results are bit-identical.'"""
    s = setup(name)
    assert s.c["pool"] == "lds" and s.B == 3 and s.desc.stage1_stride <= RC.POOL_LDS_MAX
    lds = s.pool(s.desc, s.image, null_fill, "sln_refine_pool, LDS route")
    wide = _copy(s.desc)
    keep = []
    for field, dtype in (("s1_i0", torch.int32), ("s1_i1", torch.int32), ("s1_l1", torch.float32)):
        old = s.rl._keep[{"s1_i0": 3, "s1_i1": 4, "s1_l1": 5}[field]]
        assert old.dtype == dtype and tuple(old.shape) == (s.ns, s.desc.stage1_stride) and old.data_ptr() == getattr(s.desc, field)
        new = torch.zeros(s.ns, 104, dtype=dtype, device="cuda")
        new[:, :old.shape[1]] = old
        keep.append(new)
        setattr(wide, field, new.data_ptr())
    wide.stage1_stride = 104
    plain = s.pool(wide, s.image, null_fill, "sln_refine_pool, stride 104")
    assert _bits(plain, lds), "pool_kernel and pool_lds_kernel differ in %d of %d elements" % (int((plain != lds).sum()), lds.numel())
    print("%s null_fill %d: pool_kernel == pool_lds_kernel in all %d elements" % (name, null_fill, lds.numel()))


# ----------------------------------------------------------------------------------------------------- 3. labels and counts
@pytest.mark.parametrize("name", RC.NAMES)
def test_labels_and_counts_equal_the_reference_exactly(name):
    s = setup(name)
    R = pkg("host.refine")
    c, rl = s.c, s.rl
    want, vp = RC.masked_labels(name)
    assert torch.equal(rl.labels.cpu().long(), want), "%d labels differ; route: %s" % (int((rl.labels.cpu().long() != want).sum()), s.route)
    if vp is None:
        cnt = (want >= 0).sum(dim=(2, 3) if c["per_room"] else (0, 2, 3)).to(F32)
        assert _bits(rl.inv_count.cpu(), 1.0 / cnt)
        assert rl.valid_pooled is None and rl.mask_count is None and rl.mask_status is None
    else:
        plain = RC.labels_of(RC.clean_target(s.ops), c["sizes"], F64)
        m = R.mask_counts_torch(s.ops["valid"], plain, c["per_room"], c["sizes"])
        assert torch.equal(rl.valid_pooled.cpu(), m["valid_pooled"]) and torch.equal(rl.valid_pooled.cpu() != 0, vp)
        assert torch.equal(rl.labels.cpu(), m["labels"])
        assert _bits(rl.inv_count.cpu(), m["inv_count"].contiguous()), (rl.inv_count.cpu(), m["inv_count"])
        assert torch.equal(rl.mask_count.cpu(), m["depth_count"]) and torch.equal(rl.mask_status.cpu(), m["mask_status"])
        assert bool((rl.mask_status.cpu() == (3 if RC.is_all_invalid(c) else 0)).all())


# ----------------------------------------------------------------- 4. - 6., 8. loss values, gradient (both backward kernels), report
def _check_gradient(s, got, ref, what):
    """every element of the gradient image against 1.5 x the fp64 gradient; the elements that must be exactly 0"""
    c, ops = s.c, s.ops
    Cc = c["C"]
    line = _close(got[:, :Cc], 1.5 * ref["grad64"], 1.5 * ref["grad32"].double(), what, s.route)
    g = got.cpu()
    assert float(g[:, 0].abs().max()) == 0.0, "plane 0"
    assert float(g[:, Cc - 1][ops["null"]].abs().max()) == 0.0, "null pixels of the last depth plane"
    if c["extra_channels"]:
        assert g.shape[1] == Cc + c["extra_channels"] and float(g[:, Cc:].abs().max()) == 0.0, "channels behind dep0 + n_dep"
    if ops["valid"] is not None:
        under = (ops["valid"] == 0)[:, None].expand_as(g)
        assert float(g[under].abs().max() if under.any() else 0.0) == 0.0, "pixels under the mask"
    if not RC.is_all_invalid(c):
        assert float(g[:, 1:41].abs().max()) > 0 and float(g[:, 41:Cc].abs().max()) > 0
    return line


@pytest.mark.parametrize("name", RC.NAMES)
def test_loss_gradient_and_report_against_fp64(name):
    s = setup(name)
    c, ref = s.c, RC.reference(name)
    lines = []
    # 4. the loss triple(s)
    loss = s.forward(s.desc, s.image, "sln_refine_loss_forward(%s)" % name)
    for k, part in enumerate(("total", "depth", "semantic")):
        lines.append(_close(loss[..., k], ref["loss64"][..., k], ref["loss32"][..., k], part, s.route))
    # 5. the gradient: every element, grad_scale 1.5; a second backward from the same forward gives the same bits
    scale = torch.full((1,), 1.5, device="cuda")
    grad = s.backward(s.desc, scale, "sln_refine_loss_backward(%s)" % name)
    lines.append(_check_gradient(s, grad, ref, "gradient[%s]" % c["backward"]))
    again = s.backward(s.desc, scale, "sln_refine_loss_backward(%s), again" % name)
    assert _bits(again, grad), "a second backward from the same forward differs"
    # 6. the generic kernel where the geometry picks the separable one
    if c["backward"] == "separable":
        generic = _copy(s.desc)
        generic.max_col_entries = 0
        g2 = s.backward(generic, scale, "sln_refine_loss_backward(%s), generic" % name)
        lines.append(_check_gradient(s, g2, ref, "gradient[generic, forced]"))
    # 8. the report, from the partial sums this forward left in the workspace
    nsc = int(s.lib.sln_refine_report_scratch_doubles(s.B))
    scratch, out = _full(nsc, torch.float64), _full(3 * s.B)
    tdepth = RC.clean_target(s.ops)[:, 41:].contiguous().cuda()
    if s.valid is not None:                                      # the report does not read the target under the mask either
        tdepth = s.ops["target"][:, 41:].contiguous().cuda()
    rc = s.lib.sln_refine_report(s.desc, s.L.ptr(s.image), s.L.ptr(tdepth), s.L.ptr(s.ws), s.L.ptr(scratch), None, s.L.ptr(out), s.sp())
    _sync("sln_refine_report(%s)" % name)
    if c["report"] and (c["per_room"] or s.B == 1):
        assert rc == 0, rc
        _tail_ok(out, 3 * s.B, "report"); _tail_ok(scratch, nsc, "report scratch"); s.ws_ok("report")
        rep = out[:3 * s.B].view(s.B, 3).cpu()
        assert bool(torch.isnan(rep[:, 0]).all()), "iou without iou_mean is NaN"
        r64, r32 = RC.report_reference(name, F64), RC.report_reference(name, F32)
        lines.append(_close(rep[:, 1], r64[:, 0], r32[:, 0], "depth_l1", s.route))
        lines.append(_close(rep[:, 2], r64[:, 1], r32[:, 1], "ce_last", s.route))
    else:
        assert rc == E_UNSUPPORTED, rc
        assert bool((out == SENT).all()) and bool((scratch == SENT).all()), "a refused report wrote something"
        lines.append("report refused (P * P %% 128 = %d%s)" % ((s.P * s.P) % 128, "" if c["per_room"] or s.B == 1 else ", a batch"))
    print("\n".join("%s: %s" % (name, l) for l in lines) + "\nroute: " + s.route)


# ------------------------------------------------------------------------------------------------------------- 7. live_planes
def _flagged_image(s):
    """the case's iterate with planes made dead - semantic and depth-hot planes of zeros, a depth-hot plane of ones - and the flags read off
    it as sln_scene_live_channels would write them (zeros: 0, a depth-hot plane of ones: 1, else 3)"""
    img = s.ops["image"].clone()
    B = img.shape[0]
    for b in range(B):
        img[b, [2 + b, 17, 40 - b]] = 0.0
        img[b, [41 + 3 * b, 55]] = 0.0
    img[1, 60] = 1.0                                             # room 1's null block now sums to >= 1: not null, but only for a mask that counts the flag
    # (the last depth-hot plane, which the null fill goes to, is never flagged dead: sln_scene_live_channels gives it 3)
    live = torch.full(img.shape[:2], 3, dtype=torch.uint8)
    for b in range(B):
        for ch in range(1, 70):
            if not bool(img[b, ch].any()):
                live[b, ch] = 0
            elif ch >= 41 and bool((img[b, ch] == 1.0).all()):
                live[b, ch] = 1
    assert (live[:, 1:41] == 0).any() and (live[:, 41:] == 0).any() and (live[1, 41:] == 1).sum() == 1 and int((live != 3).sum()) == 5 * B + 1 and bool((live[:, 69] == 3).all())
    dsum = img[:, 41:].double().sum(1)
    assert float((dsum - 0.5).abs().min()) >= 0.05
    null = dsum < 0.5
    assert bool(null[0].any()) and not bool(null[1].any()) and bool(null[2].any())
    dead = (live != 3)[:, :, None, None].expand_as(img)
    poisoned = torch.where(dead, torch.full_like(img, float("nan")), img)      # what a call that honours the flags must not read
    return img.cuda(), poisoned.cuda(), live, null.to(torch.uint8).cuda()


def _flag_runs(s, honoured):
    img, poisoned, live, null = _flagged_image(s)
    live_dev = live.cuda()
    scale = torch.full((1,), 1.5, device="cuda")
    assert s.lib.sln_refine_loss_live_ok(C.byref(s.desc)) == int(honoured)
    loss0 = s.forward(s.desc, img, "forward, no flags").clone()
    grad0 = s.backward(s.desc, scale, "backward, no flags")
    assert bool(torch.isfinite(loss0).all()) and not bool((grad0 == SENT).any())
    ones = s.rl.pooled_ones()
    _sync("pooled_ones")
    written = ((live & 2) != 0)
    for what, with_tables in (("flags alone", False), ("flags, null_mask and pooled_ones", True)):
        d = _copy(s.desc)
        d.live_planes = live_dev.data_ptr()
        if with_tables:
            d.null_mask, d.pooled_ones = null.data_ptr(), ones.data_ptr()
        s.ws.fill_(WS_FILL)                                      # nothing of the unflagged call is left for a plane that is skipped
        loss = s.forward(d, poisoned if honoured else img, "forward, " + what)
        assert _bits(loss, loss0), "%s: loss %s, without flags %s" % (what, loss.tolist(), loss0.tolist())
        grad = s.backward(d, scale, "backward, " + what)
        if honoured:
            assert bool((grad.cpu()[~written] == SENT).all()), "%s: a plane nobody reads the gradient of was written" % what
            assert _bits(grad.cpu()[written], grad0.cpu()[written]), what
        else:
            assert _bits(grad, grad0), "%s: the flags changed something on a route that ignores them" % what
    return int((~written).sum())


def test_live_planes_on_the_route_that_honours_them():
    """(40, (8, 12, 16)), three rooms: with the flags - alone, and with null_mask and pooled_ones - the loss bits are the unflagged
    call's although the dead planes of the image hold NaN, planes with bit 1 clear keep SENT, every other gradient plane its bits"""
    s = setup("s40-b3-rooms")
    n = _flag_runs(s, honoured=True)
    print("live_planes honoured: %d of %d gradient planes left alone; route: %s" % (n, s.B * s.C, s.route))


def test_live_planes_change_nothing_where_the_route_ignores_them():
    """(40, (12, 20, 32)): the CSR rows are too long for the separable backward kernel, sln_refine_loss_live_ok is 0, and the same flags
    must change nothing at all - every plane is read, every gradient plane written"""
    s = setup("generic-b3-batch")
    _flag_runs(s, honoured=False)
    print("live_planes ignored; route: %s" % s.route)
