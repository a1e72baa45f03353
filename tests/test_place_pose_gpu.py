"""sln_place_pose_step_views at operand level (csrc/placement.hip; DESIGN §4 "Camera poses of the target views"): the two rooms, the cameras and
the face gradients of tests/pose_refine_cases.py.  The gradient is held to tests/pose_refine_ref.py's fp64 restatement on the kernel's own
float32 operands - the placed corners are read off sln_place_forward_views through three axis cameras, whose z output IS a world coordinate -
the update to ``reproject.pose_step_torch`` on the kernel's own gradient."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import pkg

import pose_refine_cases as PC
import pose_refine_ref as PR

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
PAD = 64                 # sentinel elements in front of and behind the camera table, the master and the gradient
ROT, TRANS = 1e-5, 1e-4  # |omega| of a few 1e-3 rad, |tau| of a few 1e-3 on these gradients


def _f32(x):
    return float(np.float32(x))


class Bufs:
    """the operands of one call over both rooms (image b = r * V + v): the placement table of tests/test_place_views_gpu.py and, between
    sentinels, the camera table [R * V] of (K[9], R[9], t[3]), the float64 master [R * V, 12] = double(table entry) and grad_pose [R * V, 6]"""

    def __init__(self, which, descs=None, cams=None, seed=1):
        L = pkg("_lib")
        rooms = PC.rooms("cuda")
        cams = PC.cameras(which, "cuda") if cams is None else cams
        self.R, self.V = len(rooms), len(cams[0])
        R, V = self.R, self.V
        self.rows = [int(rm[1].shape[0]) for rm in rooms]
        self.row0 = [sum(self.rows[:r]) for r in range(R)]
        self.N, self.n_max = sum(self.rows), max(self.rows)
        self.F = [rm[3].desc.F for rm in rooms]
        self.F2 = 2 * max(self.F)
        self.stride = 9 * self.F2
        B = R * V
        f32 = dict(dtype=torch.float32, device="cuda")
        self.faces = torch.full((B, self.F2, 3, 3), SENTINEL, **f32)
        self.g_boxes, self.g_idx = torch.full((self.N, 6), SENTINEL, **f32), torch.full((self.N,), SENTINEL, **f32)
        self.g_faces = PC.grad_faces(V, "cuda", seed)
        assert tuple(self.g_faces.shape) == (B, self.F2, 3, 3)
        self.boxes, self.idx = torch.cat([rm[1] for rm in rooms]).contiguous(), torch.cat([rm[2] for rm in rooms]).contiguous()
        self.sizes = torch.full((R, max(rm[3].n_vis for rm in rooms), 3), SENTINEL, **f32)
        self.size_loss = torch.full((R,), SENTINEL, **f32)
        self.g_size_loss = torch.full((1,), 3.0, **f32)
        tab = (L.SlnPlacementRoom * R)()
        for r, rm in enumerate(rooms):
            e, a = tab[r], self.row0[r]
            e.P = rm[3].desc if descs is None else descs[r]
            e.boxes, e.angles, e.size_target = self.boxes.data_ptr() + 24 * a, self.idx.data_ptr() + 4 * a, rm[4].data_ptr()
            e.faces_out, e.sizes, e.size_loss = self.faces[r * V].data_ptr(), self.sizes[r].data_ptr(), self.size_loss.data_ptr() + 4 * r
            e.grad_faces, e.grad_size_loss = self.g_faces[r * V].data_ptr(), self.g_size_loss.data_ptr()
            e.grad_boxes, e.grad_angles = self.g_boxes.data_ptr() + 24 * a, self.g_idx.data_ptr() + 4 * a
        self.tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
        table = torch.stack([torch.cat([x.reshape(-1).float() for x in cam]) for room in cams for cam in room])          # [B, 21]
        self._cams = torch.full((2 * PAD + 21 * B,), SENTINEL, **f32)
        self.cams = self._cams[PAD:PAD + 21 * B].view(B, 21)
        self.cams.copy_(table)
        self._pose = torch.full((2 * PAD + 12 * B,), SENTINEL, dtype=torch.float64, device="cuda")
        self.pose = self._pose[PAD:PAD + 12 * B].view(B, 12)
        self.pose.copy_(self.cams[:, 9:].double())
        self._grad = torch.full((2 * PAD + 6 * B,), SENTINEL, dtype=torch.float64, device="cuda")
        self.grad = self._grad[PAD:PAD + 6 * B].view(B, 6)
        self.start = (self._cams.clone(), self._pose.clone())

    def place(self, forward=True, backward=True):
        L = pkg("_lib")
        lib, st = L.lib(), L.current_stream_ptr()
        if forward:
            L.check(lib.sln_place_forward_views(L.ptr(self.tab), L.ptr(self.cams), self.R, self.V, self.F2 // 2, self.stride, st), "sln_place_forward_views")
        if backward:
            L.check(lib.sln_place_backward_views(L.ptr(self.tab), L.ptr(self.cams), self.R, self.V, self.n_max, self.stride, st), "sln_place_backward_views")
        return self

    def step(self, rot=0.0, trans=0.0, free=None):
        L = pkg("_lib")
        self.free = None if free is None else torch.tensor(free, dtype=torch.uint8, device="cuda")
        L.check(L.lib().sln_place_pose_step_views(L.ptr(self.tab), L.ptr(self.cams), L.ptr(self.pose), L.ptr(self.grad), L.ptr(self.free), self.R, self.V,
                                                  self.stride, rot, trans, L.current_stream_ptr()), "sln_place_pose_step_views")
        return self

    def placement_outputs(self):
        return dict(faces=self.faces, sizes=self.sizes, size_loss=self.size_loss, g_boxes=self.g_boxes, g_idx=self.g_idx)

    def check_sentinels(self, grad_written=True):
        torch.cuda.synchronize()
        for name, buf in (("cams", self._cams), ("pose", self._pose), ("grad_pose", self._grad)):
            assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), "a write in front of or behind %s" % name
        if grad_written:
            assert not bool((self.grad == SENTINEL).any()), "grad_pose: an element was not written"
        else:
            assert bool((self.grad == SENTINEL).all()), "grad_pose was written"

    def untouched(self, b=None):
        """the table and the master (row b, or all of both buffers, sentinels included) hold the bits they started with"""
        torch.cuda.synchronize()
        c0, p0 = self.start
        if b is None:
            return torch.equal(self._cams.view(torch.int32), c0.view(torch.int32)) and torch.equal(self._pose.view(torch.int64), p0.view(torch.int64))
        return (torch.equal(self.cams[b].view(torch.int32), c0[PAD:-PAD].view(-1, 21)[b].view(torch.int32)) and
                torch.equal(self.pose[b].view(torch.int64), p0[PAD:-PAD].view(-1, 12)[b].view(torch.int64)))


def _bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


@functools.lru_cache(maxsize=None)
def _placed_corners():
    """per room [F, 3 corners, 3] float32 on the host: the corners as the kernels place them, by bits.  Three views whose camera has row 2 of R =
    e_j, t = 0: the z the forward stores is p . e_j + 0 = p_j exactly; cull_eps far below every coordinate keeps every face."""
    rooms = PC.rooms("cuda")
    descs = []
    for rm in rooms:
        d = type(rm[3].desc).from_buffer_copy(rm[3].desc)
        d.cull_eps = -1e30
        descs.append(d)
    axis = []
    for j in range(3):
        Rj = torch.zeros(3, 3); Rj[2, j] = 1.0
        axis.append((torch.eye(3), Rj, torch.zeros(3)))
    b = Bufs(None, descs=descs, cams=[axis] * len(rooms)).place(backward=False)
    torch.cuda.synchronize()
    out = [torch.stack([b.faces[r * 3 + j, :b.F[r], :, 2] for j in range(3)], -1).cpu().numpy() for r in range(b.R)]
    for r, rm in enumerate(rooms):       # the torch placement agrees to float32 rounding: the right vertices, the right order
        ref = rm[3].place(rm[1], rm[2])[0][0][rm[3].faces].detach().cpu().numpy()
        assert np.abs(out[r] - ref).max() <= 1e-5 * np.abs(ref).max(), "room %d" % r
    return out


@functools.lru_cache(maxsize=None)
def _reference(which):
    """per image b: (g64 [6], S [6], n) of pose_refine_ref on the kernel's operands"""
    rooms, cams = PC.rooms("cuda"), PC.cameras(which, "cuda")
    V = len(cams[0])
    gf = PC.grad_faces(V, "cpu").numpy()
    out = []
    for r, rm in enumerate(rooms):
        d, F = rm[3].desc, rm[3].desc.F
        corners = _placed_corners()[r].reshape(3 * F, 3)
        for v, (K, Rm, t) in enumerate(cams[r]):
            out.append(PR.pose_grad_ref(np.arange(3 * F).reshape(F, 3), corners, K.numpy(), Rm.numpy(), t.numpy(), gf[r * V + v, :2 * F], d.orig_size,
                                        d.proj_eps, d.cull_eps)[:3])
    return out


def test_gradient_against_the_fp64_restatement_and_nothing_else_is_written():
    b = Bufs("three").step()
    b.check_sentinels()
    assert b.untouched(), "steps 0: the camera table or the master was written"
    got, worst = b.grad.cpu().numpy(), 0.0
    for i, (g64, S, n) in enumerate(_reference("three")):
        tol = PR.pose_bound(S, n)
        ratio = np.abs(got[i] - g64) / tol
        worst = max(worst, float(ratio.max()))
        print("room %d view %d: n = %d corners, |kernel - fp64| / bound per element %s, gradient %s" %
              (i // 3, i % 3, n, np.array2string(ratio, precision=4), np.array2string(g64, precision=4)))
        assert n > 0 and np.abs(g64).min() > 0
        assert (np.abs(got[i] - g64) <= tol).all(), "room %d view %d" % (i // 3, i % 3)
    print("worst ratio %.4f" % worst)
    counts = [n for _, _, n in _reference("three")]
    assert counts[1] == 3 * b.F[0] and counts[4] == 3 * b.F[1] and 0 < counts[2] < 3 * b.F[0] and 0 < counts[5] < 3 * b.F[1]


def test_a_view_that_culls_every_face_gives_exactly_zero():
    b = Bufs("away").step(ROT, TRANS)
    b.check_sentinels()
    got = b.grad.cpu().numpy()
    for r in range(b.R):
        assert _reference("away")[2 * r][2] == 0
        assert not got[2 * r].any() and not np.signbit(got[2 * r]).any(), "room %d" % r
        assert (np.abs(got[2 * r + 1] - _reference("away")[2 * r + 1][0]) <= PR.pose_bound(*_reference("away")[2 * r + 1][1:])).all()
        # a zero gradient steps the pose by the identity: the master keeps its value (E = I exactly, tau = -0)
        assert torch.equal(b.pose[2 * r], b.start[1][PAD:-PAD].view(-1, 12)[2 * r])
        assert not b.untouched(2 * r + 1)


@pytest.mark.parametrize("rot,trans", [(ROT, TRANS), (1e-12, 0.0), (0.0, TRANS)], ids=["rodrigues", "series", "translation-only"])
def test_the_update_is_pose_step_torch_on_the_kernels_gradient(rot, trans):
    RP = pkg("host.reproject")
    free = [1, 0, 1, 1, 1, 0]
    b = Bufs("three").step(rot, trans, free)
    b.check_sentinels()
    g = b.grad.cpu()
    zero = Bufs("three").step()
    assert _bits(b.grad, zero.grad), "the gradient depends on the steps"
    start = b.start[1][PAD:-PAD].view(-1, 12).cpu()
    om, ta = -_f32(rot) * g[:, :3], -_f32(trans) * g[:, 3:]
    if rot == ROT:
        assert float(om.norm(dim=1).min()) > 1e-4
    elif rot > 0:
        assert 0 < float(om.norm(dim=1).max()) < RP.SMALL_ANGLE
    Rm, t = RP.pose_step_torch(start[:, :9].view(-1, 3, 3), start[:, 9:], om, ta)
    want = torch.cat((Rm.reshape(-1, 9), t), 1)
    got, table, table0 = b.pose.cpu(), b.cams.cpu(), b.start[0][PAD:-PAD].view(-1, 21).cpu()
    for i, fr in enumerate(free):
        if not fr:
            assert b.untouched(i), "image %d is not free: its table entry or its master was written" % i
            continue
        err = float((got[i] - want[i]).abs().max())
        print("image %d: max |master - pose_step_torch| = %.3e, moved by %.3e" % (i, err, float((got[i] - start[i]).abs().max())))
        assert err <= 1e-12
        assert not torch.equal(got[i], start[i])
        assert _bits(table[i, 9:], got[i].float()), "image %d: the table entry is not float32(master)" % i
        assert _bits(table[i, :9], table0[i, :9]), "image %d: K was written" % i
        if rot == 0.0:
            assert _bits(got[i, :9], start[i, :9]), "a pure translation changed the rotation"
    again = Bufs("three").step(rot, trans, free)
    torch.cuda.synchronize()
    assert _bits(again._grad, b._grad) and _bits(again._pose, b._pose) and _bits(again._cams, b._cams), "two calls differ"


def test_refusals_launch_nothing():
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    b = Bufs("three")
    tab, cm, ps, gr = L.ptr(b.tab), L.ptr(b.cams), L.ptr(b.pose), L.ptr(b.grad)
    s, nan, inf = b.stride, float("nan"), float("inf")
    bad = [(None, cm, ps, gr, None, 2, 3, s, ROT, TRANS), (tab, None, ps, gr, None, 2, 3, s, ROT, TRANS), (tab, cm, None, gr, None, 2, 3, s, ROT, TRANS),
           (tab, cm, ps, None, None, 2, 3, s, ROT, TRANS), (tab, cm, ps, gr, None, 0, 3, s, ROT, TRANS), (tab, cm, ps, gr, None, -1, 3, s, ROT, TRANS),
           (tab, cm, ps, gr, None, 2, 0, s, ROT, TRANS), (tab, cm, ps, gr, None, 2, -3, s, ROT, TRANS), (tab, cm, ps, gr, None, 2, 65, s, ROT, TRANS),
           (tab, cm, ps, gr, None, 2, 3, 17, ROT, TRANS), (tab, cm, ps, gr, None, 2, 3, s, -ROT, TRANS), (tab, cm, ps, gr, None, 2, 3, s, ROT, -TRANS),
           (tab, cm, ps, gr, None, 2, 3, s, nan, TRANS), (tab, cm, ps, gr, None, 2, 3, s, ROT, nan), (tab, cm, ps, gr, None, 2, 3, s, inf, TRANS),
           (tab, cm, ps, gr, None, 2, 3, s, ROT, inf)]
    for args in bad:
        assert lib.sln_place_pose_step_views(*args, st) == -1, args
    b.check_sentinels(grad_written=False)
    assert b.untouched()
    assert lib.sln_place_pose_step_views(tab, cm, ps, gr, None, 2, 3, s, ROT, TRANS, st) == 0
    b.check_sentinels()
    assert not b.untouched()


def test_a_captured_replay_equals_the_eager_bits():
    free = [1, 1, 0, 1, 1, 1]
    eager = Bufs("three").place().step(ROT, TRANS, free)
    graph = Bufs("three")
    graph.free = torch.tensor(free, dtype=torch.uint8, device="cuda")
    L = pkg("_lib")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                          # (the capturing stream is the current one inside)
        graph.place()
        L.check(L.lib().sln_place_pose_step_views(L.ptr(graph.tab), L.ptr(graph.cams), L.ptr(graph.pose), L.ptr(graph.grad), L.ptr(graph.free), 2, 3,
                                                  graph.stride, ROT, TRANS, L.current_stream_ptr()), "sln_place_pose_step_views")
    torch.cuda.synchronize()
    assert bool((graph.grad == SENTINEL).all()) and graph.untouched(), "the capture itself ran the kernel"
    g.replay()
    graph.check_sentinels()
    assert _bits(graph._grad, eager._grad) and _bits(graph._pose, eager._pose) and _bits(graph._cams, eager._cams)
    for name, got in graph.placement_outputs().items():
        assert _bits(got, eager.placement_outputs()[name]), name


def test_the_placement_kernels_give_their_bits_in_both_call_orders():
    """forward / backward alone, forward - backward - pose step, and pose step - forward - backward on the same operands: the placement's outputs
    by bits, and one pose gradient (it reads none of them); after a real step the placement through the stepped table is the placement
    through a fresh table that holds the stepped cameras"""
    base = Bufs("three").place()
    after = Bufs("three").place().step()
    before = Bufs("three").step().place()
    torch.cuda.synchronize()
    for name, want in base.placement_outputs().items():
        assert not bool((want == SENTINEL).all())
        assert _bits(after.placement_outputs()[name], want) and _bits(before.placement_outputs()[name], want), name
    assert _bits(after.grad, before.grad)
    moved = Bufs("three").place().step(ROT, TRANS).place()
    torch.cuda.synchronize()
    cams = [[tuple(moved.cams[r * 3 + v, a:e].cpu() for a, e in ((0, 9), (9, 18), (18, 21))) for v in range(3)] for r in range(2)]
    fresh = Bufs(None, cams=cams).place()
    torch.cuda.synchronize()
    for name, want in fresh.placement_outputs().items():
        assert _bits(moved.placement_outputs()[name], want), name
    assert not _bits(moved.faces, base.faces)
