"""sln_place_camera_step_views at operand level (csrc/placement.hip; DESIGN §4 "Intrinsics of the target views"): the two rooms, the cameras, the
face gradients and the buffers of tests/test_place_pose_gpu.py, with the float64 master of the intrinsics [R * V, 4] = (fx, fy, cx, cy) and
grad_intr [R * V, 4] between sentinels of their own.  The gradient is held to tests/intrinsics_refine_ref.py's fp64 restatement on the
kernel's own float32 operands, the update to ``reproject.intrinsics_step_torch`` on the kernel's own gradient, the pose half of the call to
sln_place_pose_step_views by bits."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg

import intrinsics_refine_ref as IR
import pose_refine_cases as PC
import test_place_pose_gpu as TP
from test_place_pose_gpu import PAD, ROT, SENTINEL, TRANS, _bits, _f32

pytestmark = pytest.mark.gpu

# the entries of d fx, d fy, d cx, d cy on these random face gradients are 0.01 - 0.6 (tests/test_intrinsics_refine_host.py prints them): a
# focal step that changes a focal length of some hundred pixels by a part in 1e4 - 1e2, a centre step that moves the principal point by
# a fraction of a pixel - both far above the float32 rounding of the table's entries
FOCAL, CENTER = 1e-4, 1.0
KIDX = [0, 4, 2, 5]      # fx, fy, cx, cy in the table's K[9]


class Bufs(TP.Bufs):
    def __init__(self, which, **kw):
        super().__init__(which, **kw)
        B = self.R * self.V
        self._intr = torch.full((2 * PAD + 4 * B,), SENTINEL, dtype=torch.float64, device="cuda")
        self.intr = self._intr[PAD:PAD + 4 * B].view(B, 4)
        self.intr.copy_(self.cams[:, KIDX].double())
        self._gintr = torch.full((2 * PAD + 4 * B,), SENTINEL, dtype=torch.float64, device="cuda")
        self.gintr = self._gintr[PAD:PAD + 4 * B].view(B, 4)
        self.intr0 = self._intr.clone()
        self.free = self.ifree = None

    def camera_step(self, rot=0.0, trans=0.0, focal=0.0, center=0.0, tie=True, free=None, ifree=None, intr=True):
        L = pkg("_lib")
        self.free = None if free is None else torch.tensor(free, dtype=torch.uint8, device="cuda")
        self.ifree = None if ifree is None else torch.tensor(ifree, dtype=torch.uint8, device="cuda")
        L.check(L.lib().sln_place_camera_step_views(*self.args(intr), self.R, self.V, self.stride, rot, trans, focal, center, int(tie),
                                                    L.current_stream_ptr()), "sln_place_camera_step_views")
        return self

    def args(self, intr=True):
        P = pkg("_lib").ptr
        return (P(self.tab), P(self.cams), P(self.pose), P(self.grad), P(self.free)) + ((P(self.intr), P(self.gintr), P(self.ifree)) if intr else (None,) * 3)

    def check_sentinels(self, grad_written=True, intr_written=True):
        super().check_sentinels(grad_written)
        for name, buf in (("intr", self._intr), ("grad_intr", self._gintr)):
            assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), "a write in front of or behind %s" % name
        if intr_written:
            assert not bool((self.gintr == SENTINEL).any()), "grad_intr: an element was not written"
        else:
            assert bool((self.gintr == SENTINEL).all()), "grad_intr was written"

    def intr_untouched(self, b=None):
        """the master of the intrinsics (row b, or the whole buffer, sentinels included) holds the bits it started with"""
        torch.cuda.synchronize()
        if b is None:
            return torch.equal(self._intr.view(torch.int64), self.intr0.view(torch.int64))
        return torch.equal(self.intr[b].view(torch.int64), self.intr0[PAD:-PAD].view(-1, 4)[b].view(torch.int64))

    def table0(self):
        return self.start[0][PAD:-PAD].view(-1, 21)


@functools.lru_cache(maxsize=None)
def _reference(which):
    """per image b: (g64 [4], S [4], n) of intrinsics_refine_ref on the kernel's operands (the placed corners by bits)"""
    rooms, cams = PC.rooms("cuda"), PC.cameras(which, "cuda")
    V = len(cams[0])
    gf = PC.grad_faces(V, "cpu").numpy()
    out = []
    for r, rm in enumerate(rooms):
        d, F = rm[3].desc, rm[3].desc.F
        corners = TP._placed_corners()[r].reshape(3 * F, 3)
        for v, (K, Rm, t) in enumerate(cams[r]):
            out.append(IR.intr_grad_ref(np.arange(3 * F).reshape(F, 3), corners, K.numpy(), Rm.numpy(), t.numpy(), gf[r * V + v, :2 * F], d.orig_size,
                                        d.proj_eps, d.cull_eps)[:3])
    return out


def test_gradient_against_the_fp64_restatement_and_nothing_else_is_written():
    b = Bufs("three").camera_step()
    b.check_sentinels()
    assert b.untouched() and b.intr_untouched(), "steps 0: the camera table or a master was written"
    got, worst = b.gintr.cpu().numpy(), 0.0
    for i, (g64, S, n) in enumerate(_reference("three")):
        tol = IR.intr_bound(S, n)
        ratio = np.abs(got[i] - g64) / tol
        worst = max(worst, float(ratio.max()))
        print("room %d view %d: n = %d corners, |kernel - fp64| / bound per element %s, gradient %s" %
              (i // 3, i % 3, n, np.array2string(ratio, precision=4), np.array2string(g64, precision=4)))
        assert n > 0 and np.abs(g64).min() > 0
        assert (np.abs(got[i] - g64) <= tol).all(), "room %d view %d" % (i // 3, i % 3)
    print("worst ratio %.4f" % worst)
    counts = [n for _, _, n in _reference("three")]
    assert counts[1] == 3 * b.F[0] and counts[4] == 3 * b.F[1] and 0 < counts[2] < 3 * b.F[0] and 0 < counts[5] < 3 * b.F[1]
    pose = TP.Bufs("three").step()
    torch.cuda.synchronize()
    assert _bits(b._grad, pose._grad), "grad_pose is not sln_place_pose_step_views' by bits"


def test_a_view_that_culls_every_face_gives_exactly_zero():
    b = Bufs("away").camera_step(ROT, TRANS, FOCAL, CENTER)
    b.check_sentinels()
    got = b.gintr.cpu().numpy()
    for r in range(b.R):
        assert _reference("away")[2 * r][2] == 0
        assert not got[2 * r].any() and not np.signbit(got[2 * r]).any(), "room %d" % r
        assert (np.abs(got[2 * r + 1] - _reference("away")[2 * r + 1][0]) <= IR.intr_bound(*_reference("away")[2 * r + 1][1:])).all()
        # a zero gradient steps by the identity: exp(-0) = 1, cx - 0
        assert b.intr_untouched(2 * r) and not b.intr_untouched(2 * r + 1)
        assert _bits(b.cams[2 * r, :9], b.table0()[2 * r, :9])


@pytest.mark.parametrize("rot,trans,free", [(ROT, TRANS, [1, 0, 1, 1, 1, 0]), (0.0, 0.0, None), (0.0, TRANS, None)], ids=["steps", "steps-0", "translation"])
def test_null_intrinsics_pointers_make_the_call_the_pose_entry_point(rot, trans, free):
    a = Bufs("three").camera_step(rot, trans, FOCAL, CENTER, free=free, intr=False)
    p = TP.Bufs("three").step(rot, trans, free)
    a.check_sentinels(intr_written=False)
    assert a.intr_untouched()
    assert _bits(a._grad, p._grad) and _bits(a._pose, p._pose) and _bits(a._cams, p._cams)
    assert a.untouched() == (rot == 0.0 and trans == 0.0)


def test_steps_zero_and_a_held_view_leave_master_and_table_untouched():
    zero = Bufs("three").camera_step(0.0, 0.0, 0.0, 0.0)
    zero.check_sentinels()
    assert zero.untouched() and zero.intr_untouched()
    held = [1, 0, 1, 0, 1, 1]
    b = Bufs("three").camera_step(0.0, 0.0, FOCAL, CENTER, ifree=held)
    b.check_sentinels()
    assert _bits(b.gintr, zero.gintr) and _bits(b.grad, zero.grad), "the gradients depend on the steps or the flags"
    for i, fr in enumerate(held):
        assert b.untouched(i) == (not fr) and b.intr_untouched(i) == (not fr), "image %d" % i
    assert _bits(b._pose, b.start[1]), "pose steps 0: the pose master was written"
    assert _bits(b.cams[:, 9:], b.table0()[:, 9:]), "pose steps 0: R or t of the table was written"
    # the pose held, the intrinsics free and the reverse: each flag array bars its own half only
    c = Bufs("three").camera_step(ROT, TRANS, FOCAL, CENTER, free=[0] * 6, ifree=[1] * 6)
    d = Bufs("three").camera_step(ROT, TRANS, FOCAL, CENTER, free=[1] * 6, ifree=[0] * 6)
    torch.cuda.synchronize()
    assert _bits(c._pose, c.start[1]) and _bits(c.cams[:, 9:], c.table0()[:, 9:]) and not c.intr_untouched()
    assert d.intr_untouched() and _bits(d.cams[:, :9], d.table0()[:, :9]) and not _bits(d._pose, d.start[1])


@pytest.mark.parametrize("tie", [True, False], ids=["tied", "untied"])
@pytest.mark.parametrize("focal,center", [(FOCAL, CENTER), (FOCAL, 0.0), (0.0, CENTER)], ids=["both", "focal-only", "centre-only"])
def test_the_update_is_intrinsics_step_torch_on_the_kernels_gradient(focal, center, tie):
    RP = pkg("host.reproject")
    ifree = [1, 1, 0, 1, 0, 1]
    b = Bufs("three").camera_step(0.0, 0.0, focal, center, tie, ifree=ifree)
    b.check_sentinels()
    g, table0 = b.gintr.cpu(), b.table0().cpu()
    start = b.intr0[PAD:-PAD].view(-1, 4).cpu()
    assert torch.equal(start, table0[:, KIDX].double())
    K0 = table0[:, :9].double().view(-1, 3, 3)
    want = RP.intrinsics_step_torch(K0, g, _f32(focal), _f32(center), tie).reshape(-1, 9)
    got, table = b.intr.cpu(), b.cams.cpu()
    for i, fr in enumerate(ifree):
        if not fr:
            assert b.untouched(i) and b.intr_untouched(i), "image %d is not free: its table entry or its master was written" % i
            continue
        err = float((got[i] - want[i, KIDX]).abs().max())
        print("image %d: max |master - intrinsics_step_torch| = %.3e, moved by %s" % (i, err, (got[i] - start[i]).numpy()))
        assert err <= 1e-12
        assert _bits(want[i, [1, 3, 6, 7, 8]], K0[i].reshape(9)[[1, 3, 6, 7, 8]])
        assert not torch.equal(got[i], start[i])
        assert _bits(table[i, KIDX], got[i].float()), "image %d: the table's four entries are not float32(master)" % i
        assert _bits(table[i, [1, 3, 6, 7, 8]], table0[i, [1, 3, 6, 7, 8]]), "image %d: K[1], K[3] or the last row was written" % i
        assert _bits(table[i, 9:], table0[i, 9:]), "image %d: R or t was written at pose steps 0" % i
        if focal == 0.0:
            assert _bits(got[i, :2], start[i, :2]), "a centre step changed a focal length"
        if center == 0.0:
            assert _bits(got[i, 2:], start[i, 2:]), "a focal step moved the principal point"
        if tie and focal > 0:
            r0, r1 = float(start[i, 0]) / float(start[i, 1]), float(got[i, 0]) / float(got[i, 1])
            assert abs(r1 - r0) <= 5 * 2.0 ** -53 * r0, "image %d: the aspect ratio moved by more than rounding" % i
    again = Bufs("three").camera_step(0.0, 0.0, focal, center, tie, ifree=ifree)
    torch.cuda.synchronize()
    for x, y in ((again._gintr, b._gintr), (again._intr, b._intr), (again._cams, b._cams), (again._grad, b._grad), (again._pose, b._pose)):
        assert _bits(x, y), "two calls differ"


def test_both_updates_use_the_old_camera():
    """pose and intrinsics stepped in one call: each half equals that half stepped alone from a fresh copy - neither reads what the other wrote"""
    both = Bufs("three").camera_step(ROT, TRANS, FOCAL, CENTER, False)
    pose = Bufs("three").camera_step(ROT, TRANS, 0.0, 0.0, False)
    intr = Bufs("three").camera_step(0.0, 0.0, FOCAL, CENTER, False)
    for b in (both, pose, intr):
        b.check_sentinels()
    assert _bits(both._grad, pose._grad) and _bits(both._gintr, intr._gintr) and _bits(both._grad, intr._grad) and _bits(both._gintr, pose._gintr)
    assert _bits(both._pose, pose._pose) and _bits(both.cams[:, 9:], pose.cams[:, 9:]), "the pose half"
    assert _bits(both._intr, intr._intr) and _bits(both.cams[:, :9], intr.cams[:, :9]), "the intrinsics half"
    assert pose.intr_untouched() and _bits(pose.cams[:, :9], pose.table0()[:, :9]) and _bits(intr._pose, intr.start[1])
    assert not both.intr_untouched() and not _bits(both._pose, both.start[1])
    old = TP.Bufs("three").step(ROT, TRANS)
    torch.cuda.synchronize()
    assert _bits(both._pose, old._pose) and _bits(both._grad, old._grad) and _bits(both.cams[:, 9:], old.cams[:, 9:]), "the pose half against sln_place_pose_step_views"


def test_refusals_launch_nothing():
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    b = Bufs("three")
    b.ifree = torch.ones(6, dtype=torch.uint8, device="cuda")
    tab, cm, ps, gr, _, it, gi, fr = b.args()
    s, nan, inf = b.stride, float("nan"), float("inf")
    ok = dict(tab=tab, cm=cm, ps=ps, gr=gr, pf=None, it=it, gi=gi, fr=fr, R=2, V=3, s=s, rot=ROT, trans=TRANS, focal=FOCAL, center=CENTER, tie=1)
    call = lambda **kw: lib.sln_place_camera_step_views(*[dict(ok, **kw)[k] for k in ok], st)
    bad = [dict(tab=None), dict(cm=None), dict(ps=None), dict(gr=None), dict(R=0), dict(R=-1), dict(V=0), dict(V=-3), dict(V=65), dict(s=17),
           dict(rot=-ROT), dict(trans=-TRANS), dict(rot=nan), dict(trans=nan), dict(rot=inf), dict(trans=inf),            # the pose entry point's
           dict(gi=None), dict(it=None), dict(it=None, gi=None),                                                          # (the last: intr_free without intr)
           dict(focal=-FOCAL), dict(center=-CENTER), dict(focal=nan), dict(center=nan), dict(focal=inf), dict(center=inf),
           dict(it=None, gi=None, fr=None, focal=-FOCAL), dict(it=None, gi=None, fr=None, center=nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
    b.check_sentinels(grad_written=False, intr_written=False)
    assert b.untouched() and b.intr_untouched()
    assert call() == 0
    b.check_sentinels()
    assert not b.untouched() and not b.intr_untouched()


def test_a_captured_replay_equals_the_eager_bits():
    free, ifree = [1, 1, 0, 1, 1, 1], [1, 0, 1, 1, 1, 1]
    eager = Bufs("three").place().camera_step(ROT, TRANS, FOCAL, CENTER, True, free, ifree)
    graph = Bufs("three")
    graph.free, graph.ifree = (torch.tensor(x, dtype=torch.uint8, device="cuda") for x in (free, ifree))
    L = pkg("_lib")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                          # (the capturing stream is the current one inside)
        graph.place()
        L.check(L.lib().sln_place_camera_step_views(*graph.args(), 2, 3, graph.stride, ROT, TRANS, FOCAL, CENTER, 1, L.current_stream_ptr()),
                "sln_place_camera_step_views")
    torch.cuda.synchronize()
    assert bool((graph.gintr == SENTINEL).all()) and graph.untouched() and graph.intr_untouched(), "the capture itself ran the kernel"
    g.replay()
    graph.check_sentinels()
    for x, y in ((graph._gintr, eager._gintr), (graph._intr, eager._intr), (graph._cams, eager._cams), (graph._grad, eager._grad), (graph._pose, eager._pose)):
        assert _bits(x, y)
    for name, got in graph.placement_outputs().items():
        assert _bits(got, eager.placement_outputs()[name]), name


def test_the_placement_kernels_give_their_bits_in_both_call_orders():
    """forward / backward alone, forward - backward - camera step, and camera step - forward - backward on the same operands: the placement's
    outputs by bits, and one pair of gradients (the step reads none of them); after a real step the placement through the stepped table is
    the placement through a fresh table that holds the stepped cameras"""
    base = Bufs("three").place()
    after = Bufs("three").place().camera_step()
    before = Bufs("three").camera_step().place()
    torch.cuda.synchronize()
    for name, want in base.placement_outputs().items():
        assert not bool((want == SENTINEL).all())
        assert _bits(after.placement_outputs()[name], want) and _bits(before.placement_outputs()[name], want), name
    assert _bits(after.gintr, before.gintr) and _bits(after.grad, before.grad)
    moved = Bufs("three").place().camera_step(ROT, TRANS, FOCAL, CENTER).place()
    torch.cuda.synchronize()
    cams = [[tuple(moved.cams[r * 3 + v, a:e].cpu() for a, e in ((0, 9), (9, 18), (18, 21))) for v in range(3)] for r in range(2)]
    fresh = Bufs(None, cams=cams).place()
    torch.cuda.synchronize()
    for name, want in fresh.placement_outputs().items():
        assert _bits(moved.placement_outputs()[name], want), name
    assert not _bits(moved.faces, base.faces)
