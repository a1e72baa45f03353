"""sln_place_forward_views / sln_place_backward_views at operand level (csrc/placement.hip; DESIGN §4 "Several target views per room"):
two rooms of different row counts from the rooms and the bank of tests/test_refine_gpu.py, the placement projected through V cameras
per room.  The single-view kernels (sln_place_*_rooms) are the yardstick for bits, oracle/refine_ref.py::place_scene + raster_ref.project
in fp64 for the summed gradients."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

import test_refine_gpu as TR

pytestmark = pytest.mark.gpu

from oracle import raster_ref as rr, refine_ref     # noqa: E402

SENTINEL = 12345.0
TAIL = 64
NAMES_B = ["cabinet", "lamp", "sofa", "television", "__room__"]


def _boxes_b():
    g = torch.Generator().manual_seed(7)
    n = len(NAMES_B)
    lo = torch.rand(n, 3, generator=g) * 0.45 + 0.05
    lo[:, 1] = 0.0; lo[:, 2] = lo[:, 2] * 0.6
    boxes = torch.cat([lo, lo + torch.rand(n, 3, generator=g) * 0.2 + 0.12], 1)
    boxes[-1] = torch.tensor([0, 0, 0, 3.6, 2.5, 4.4])
    return boxes.cuda(), torch.randint(0, 24, (n,), generator=g).float().cuda()


@functools.lru_cache(maxsize=None)
def _rooms():
    """[(class names, boxes [n, 6], angle bins [n] (fractional), scene, size targets [n_vis, 3])] of the two rooms, and the bank"""
    R = pkg("host.refine")
    bank = R.MeshBank(TR.FURN, "cuda", seed=3)
    out = []
    for names, (boxes, angles) in ((TR.NAMES, TR._inputs("cuda")), (NAMES_B, _boxes_b())):
        scene = R.RefineScene(names, bank, boxes[-1].clone(), image_size=64)
        tgt = torch.stack([torch.tensor([0.5, 0.4, 0.6]) * (1 + 0.1 * k) for k in range(scene.n_vis)]).cuda().contiguous()
        out.append((names, boxes.contiguous(), (angles + 0.3).contiguous(), scene, tgt))
    assert out[0][1].shape[0] != out[1][1].shape[0] and out[0][3].desc.F != out[1][3].desc.F
    return out, bank


def _object_centre(room, k=0):
    _, boxes, _, scene, _ = room
    b, ext = boxes[int(scene.vis[k])].cpu().double(), boxes[-1, 3:].cpu().double()
    return ((b[:3] + b[3:]) / 2 * ext).numpy()


@functools.lru_cache(maxsize=None)
def _cameras(which):
    """per room a list of (K, R, t): "own" - the refinement camera; "three" - it, a look_at_view from outside the room's upper corner (sees
    everything: nothing culled) and one from the centre of the room's first object (part of that object lies behind it); "away" - a camera in
    front of the room that looks away from it (every corner behind cull_eps), then the outside one"""
    RP = pkg("host.reproject")
    cams = []
    for room in _rooms()[0]:
        ext = room[1][-1, 3:].cpu().double().numpy()
        own = RP.refine_view(room[1][-1], 64)[:3]
        outside = RP.look_at_view(ext + [1.5, 1.0, 2.0], ext / 2)[:3]
        c = _object_centre(room)
        close = RP.look_at_view(c, c + [-1.0, -0.2, -1.0])[:3]
        front = np.array([ext[0] / 2, ext[1] / 2, ext[2] + 1.0])
        away = RP.look_at_view(front, front + [0.0, 0.0, 1.0])[:3]
        cams.append(dict(own=[own], three=[own, outside, close], away=[away, outside])[which])
    return cams


class Bufs:
    """the operands of one call over both rooms: image b = r * V + v; every output starts as SENTINEL and has TAIL floats behind it"""

    def __init__(self, V, descs=None, seed=1):
        L = pkg("_lib")
        rooms = _rooms()[0]
        self.R, self.V = len(rooms), V
        self.rows = [int(rm[1].shape[0]) for rm in rooms]
        self.row0 = [sum(self.rows[:r]) for r in range(self.R)]
        self.N, self.n_max = sum(self.rows), max(self.rows)
        self.F = [rm[3].desc.F for rm in rooms]
        self.F2 = 2 * max(self.F)
        self.stride = 9 * self.F2
        B = self.R * V
        full = lambda n: torch.full((n + TAIL,), SENTINEL, device="cuda")
        self._faces, self._g_boxes, self._g_idx = full(B * self.stride), full(6 * self.N), full(self.N)
        self.faces, self.g_boxes, self.g_idx = self._faces[:B * self.stride].view(B, self.F2, 3, 3), self._g_boxes[:6 * self.N].view(-1, 6), self._g_idx[:self.N]
        self.g_faces = torch.randn(B, self.F2, 3, 3, generator=torch.Generator().manual_seed(seed)).cuda()
        self.boxes, self.idx = torch.cat([rm[1] for rm in rooms]).contiguous(), torch.cat([rm[2] for rm in rooms]).contiguous()
        self.sizes = torch.full((self.R, max(rm[3].n_vis for rm in rooms), 3), SENTINEL, device="cuda")
        self.size_loss = torch.full((self.R,), SENTINEL, device="cuda")
        self.g_size_loss = torch.full((1,), 3.0, device="cuda")
        tab = (L.SlnPlacementRoom * self.R)()
        for r, rm in enumerate(rooms):
            e, a = tab[r], self.row0[r]
            e.P = rm[3].desc if descs is None else descs[r]
            e.boxes, e.angles, e.size_target = self.boxes.data_ptr() + 24 * a, self.idx.data_ptr() + 4 * a, rm[4].data_ptr()
            e.faces_out, e.sizes, e.size_loss = self.faces[r * V].data_ptr(), self.sizes[r].data_ptr(), self.size_loss.data_ptr() + 4 * r
            e.grad_faces, e.grad_size_loss = self.g_faces[r * V].data_ptr(), self.g_size_loss.data_ptr()
            e.grad_boxes, e.grad_angles = self.g_boxes.data_ptr() + 24 * a, self.g_idx.data_ptr() + 4 * a
        self.tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()

    def cams(self, cameras):
        assert len(cameras) == self.R and all(len(c) == self.V for c in cameras)
        return torch.stack([torch.cat([x.reshape(-1).float() for x in cam]) for room in cameras for cam in room]).contiguous().cuda()

    def views(self, cams, forward=True, backward=True):
        L = pkg("_lib")
        lib, st = L.lib(), L.current_stream_ptr()
        if forward:
            L.check(lib.sln_place_forward_views(L.ptr(self.tab), L.ptr(cams), self.R, self.V, self.F2 // 2, self.stride, st), "sln_place_forward_views")
        if backward:
            L.check(lib.sln_place_backward_views(L.ptr(self.tab), L.ptr(cams), self.R, self.V, self.n_max, self.stride, st), "sln_place_backward_views")
        return self

    def single(self):
        assert self.V == 1
        L = pkg("_lib")
        lib, st = L.lib(), L.current_stream_ptr()
        L.check(lib.sln_place_forward_rooms(L.ptr(self.tab), self.R, self.F2 // 2, st), "sln_place_forward_rooms")
        L.check(lib.sln_place_backward_rooms(L.ptr(self.tab), self.R, self.n_max, st), "sln_place_backward_rooms")
        return self

    def outputs(self):
        return dict(faces=self._faces, sizes=self.sizes, size_loss=self.size_loss, g_boxes=self._g_boxes, g_idx=self._g_idx)

    def check_sentinels(self):
        """nothing behind faces, g_boxes, g_idx was written; the padded face rows of every view are untouched; everything else was written"""
        torch.cuda.synchronize()
        for name, buf in (("faces", self._faces), ("g_boxes", self._g_boxes), ("g_idx", self._g_idx)):
            assert bool((buf[-TAIL:] == SENTINEL).all()), "a write behind %s" % name
        for r in range(self.R):
            for v in range(self.V):
                img = self.faces[r * self.V + v]
                assert bool((img[2 * self.F[r]:] == SENTINEL).all()), "room %d view %d: a padded face row was written" % (r, v)
                assert not bool((img[:2 * self.F[r]] == SENTINEL).any()), "room %d view %d: a face row was not written" % (r, v)
        assert not bool((self.g_boxes == SENTINEL).any()) and not bool((self.g_idx == SENTINEL).any())
        assert not bool((self.size_loss == SENTINEL).any())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _view_descs(cameras, v):
    return [rm[3].with_view(*cameras[r][v]).desc for r, rm in enumerate(_rooms()[0])]


def _single_view(cameras, v, g_faces_of=None):
    """the single-view kernels with view v's camera in the rooms' descriptors (``RefineScene.with_view``); ``g_faces_of``: a V-view
    ``Bufs`` whose gradient images of view v are this call's"""
    one = Bufs(1, _view_descs(cameras, v))
    if g_faces_of is not None:
        for r in range(one.R):
            one.g_faces[r].copy_(g_faces_of.g_faces[r * g_faces_of.V + v])
    return one.single()


def _culled(bufs, r, v):
    """per face of room r in view v: collapsed to (0, 0, 0) (a face that is kept has z >= cull_eps in every corner)"""
    return (bufs.faces[r * bufs.V + v, :bufs.F[r]].reshape(bufs.F[r], 9) == 0).all(1)


def test_one_view_with_the_rooms_own_camera_gives_the_bits_of_the_rooms_kernels():
    cameras = _cameras("own")
    many = Bufs(1)
    many.views(many.cams(cameras))
    one = Bufs(1).single()
    many.check_sentinels(); one.check_sentinels()
    for name, got in many.outputs().items():
        assert _bits(got, one.outputs()[name]), name
    assert float(many.g_boxes.abs().max()) > 0 and float(many.g_idx.abs().max()) > 0 and float(many.size_loss.min()) > 0


def test_three_views_forward_equals_the_single_view_kernel_per_view():
    cameras = _cameras("three")
    many = Bufs(3)
    many.views(many.cams(cameras), backward=False)
    torch.cuda.synchronize()
    for v in range(3):
        one = _single_view(cameras, v)
        for r in range(many.R):
            assert _bits(many.faces[r * 3 + v], one.faces[r]), "room %d view %d" % (r, v)
        assert _bits(many.sizes, one.sizes) and _bits(many.size_loss, one.size_loss)
    rooms = _rooms()[0]
    for r, rm in enumerate(rooms):
        ptr = rm[3]._keep_static[5].cpu().tolist()                   # obj_face_ptr
        close, outside = _culled(many, r, 2), _culled(many, r, 1)
        obj0 = close[ptr[0]:ptr[1]]
        print("room %d: view 2 culls %d of %d faces (%d of object 0's %d), view 1 culls %d" %
              (r, int(close.sum()), close.numel(), int(obj0.sum()), obj0.numel(), int(outside.sum())))
        assert 0 < int(obj0.sum()) < obj0.numel(), "the close view does not cull PART of object 0"
        assert int(outside.sum()) == 0, "the outside view culls a face"
        # culled in one view only: the same faces are kept in the outside view
        assert bool((many.faces[r * 3 + 1, :many.F[r]][close].reshape(-1, 9) != 0).any(1).all())


def _oracle_gradients(bufs, cameras):
    """fp64 on the CPU, autograd: sum over the views of <faces of the view (fill_back copies included), grad_faces> + g_size_loss * size_loss
    -> per room (d boxes [n, 6], d angles [n])"""
    DR = pkg("host.diff_render")
    rooms, bank = _rooms()
    out = []
    for r, (names, boxes, angles, scene, tgt) in enumerate(rooms):
        models = {k: {kk: vv.detach().cpu().double() for kk, vv in m.items() if kk != "f"} for k, m in bank.models.items()}
        b64, a64 = boxes.detach().cpu().double().requires_grad_(True), angles.detach().cpu().double().requires_grad_(True)
        b_in = torch.cat([b64[:-1], boxes[-1:].detach().cpu().double()])
        verts, _, sl64 = refine_ref.place_scene(b_in, a64, names, models, [t.cpu().double() for t in tgt])
        allv = torch.cat([verts, scene.shell_v.cpu().double()])[None]
        Vm = scene.desc.Vm
        counts = [bank.models[names[i]]["v"].shape[0] for i in scene.vis.tolist()]
        remap = torch.full((scene.n_vis * Vm + scene.shell_v.shape[0],), -1, dtype=torch.int64)
        off = 0
        for k, c in enumerate(counts):
            remap[k * Vm:k * Vm + c] = torch.arange(off, off + c); off += c
        remap[scene.n_vis * Vm:] = torch.arange(off, off + scene.shell_v.shape[0])
        faces = remap[scene.faces.cpu()]
        assert (faces >= 0).all()
        total = float(bufs.g_size_loss[0]) * sl64
        for v, cam in enumerate(cameras[r]):
            K, Rm, t = (x.double().reshape(s) for x, s in zip(cam, ((1, 3, 3), (1, 3, 3), (1, 1, 3))))
            ref = rr.vertices_to_faces(rr.project(allv, K, Rm, t, 512), faces[None])[0]
            cam_z = (torch.matmul(allv, Rm.transpose(1, 2)) + t)[0, :, 2]
            culled = (cam_z[faces] < DR.CULL_EPS).any(1)
            ref = torch.where(culled[:, None, None], torch.zeros_like(ref), ref)
            w = bufs.g_faces[r * bufs.V + v, :2 * bufs.F[r]].cpu().double()
            total = total + (torch.cat((ref, ref[:, [2, 1, 0]])) * w).sum()
        total.backward()
        out.append((b64.grad, a64.grad))
    return out


def test_three_views_backward_against_the_fp64_object_loop():
    """the bar of test_refine_gpu.py::test_fused_placement_matches_the_restated_object_loop: rtol 2e-4, atol 2e-4 of the largest entry"""
    cameras = _cameras("three")
    many = Bufs(3)
    many.views(many.cams(cameras))
    many.check_sentinels()
    singles = [_single_view(cameras, v, many) for v in range(3)]
    # the sum of three single-view calls counts the size loss's gradient three times (boxes only): a call with zero image gradients gives
    # that term alone, taken off twice
    size_only = Bufs(1, _view_descs(cameras, 0))
    size_only.g_faces.zero_()
    size_only.single()
    torch.cuda.synchronize()
    summed_boxes = (sum(s.g_boxes.double() for s in singles) - 2.0 * size_only.g_boxes.double()).cpu()
    ref = _oracle_gradients(many, cameras)
    for r, (gb64, ga64) in enumerate(ref):
        a, n = many.row0[r], many.rows[r]
        gb, ga = many.g_boxes[a:a + n].cpu(), many.g_idx[a:a + n].cpu()
        top_b, top_a = float(gb64.abs().max()), float(ga64.abs().max())
        assert top_b > 0 and top_a > 0
        summed_a = sum(s.g_idx[a:a + n].double() for s in singles).cpu()
        print("room %d: max |d boxes - fp64| = %.3e (largest entry %.3e), max |d angles - fp64| = %.3e (largest %.3e); against the sum of "
              "three single-view calls: d boxes %.3e, d angles %.3e" %
              (r, float((gb.double() - gb64).abs().max()), top_b, float((ga.double() - ga64).abs().max()), top_a,
               float((gb.double() - summed_boxes[a:a + n]).abs().max()), float((ga.double() - summed_a).abs().max())))
        assert_close(gb.numpy(), gb64.numpy(), "d/d boxes of room %d" % r, rtol=2e-4, atol=2e-4 * top_b)
        assert_close(ga.numpy(), ga64.numpy(), "d/d angles of room %d" % r, rtol=2e-4, atol=2e-4 * top_a)
        assert float(gb[-1].abs().max()) == 0.0 and float(ga[-1].abs()) == 0.0, "the room row's gradients are exactly 0"


def test_a_view_that_sees_nothing_adds_nothing():
    cameras = _cameras("away")
    many = Bufs(2)
    many.views(many.cams(cameras))
    many.check_sentinels()
    one = _single_view(cameras, 1, many)
    torch.cuda.synchronize()
    for r in range(many.R):
        assert not bool(many.faces[2 * r, :2 * many.F[r]].any()), "room %d: view 0 has a face that is not (0, 0, 0)" % r
        assert bool(many.faces[2 * r + 1, :2 * many.F[r]].any())
        assert _bits(many.faces[2 * r + 1], one.faces[r])
    assert _bits(many.g_boxes, one.g_boxes) and _bits(many.g_idx, one.g_idx)
    assert float(many.g_idx.abs().max()) > 0


def test_refusals_launch_nothing():
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    b = Bufs(2)
    cams = b.cams(_cameras("away"))
    tab, cm = L.ptr(b.tab), L.ptr(cams)
    before = {k: v.clone() for k, v in b.outputs().items()}
    F, n, s = b.F2 // 2, b.n_max, b.stride
    bad = [(None, cm, 2, 2, F, s), (tab, None, 2, 2, F, s), (tab, cm, 0, 2, F, s), (tab, cm, 2, 0, F, s), (tab, cm, 2, 65, F, s),
           (tab, cm, 2, 2, 0, s), (tab, cm, 2, 2, F, 17), (tab, cm, -1, 2, F, s), (tab, cm, 2, -3, F, s)]
    for args in bad:
        assert lib.sln_place_forward_views(*args, st) == -1, args
        a = list(args); a[4] = n if args[4] else 0
        assert lib.sln_place_backward_views(*a, st) == -1, a
    torch.cuda.synchronize()
    for k, v in b.outputs().items():
        assert _bits(v, before[k]), "%s was written by a refused call" % k
    assert lib.sln_place_forward_views(tab, cm, 2, 2, F, s, st) == 0 and lib.sln_place_backward_views(tab, cm, 2, 2, n, s, st) == 0
    b.check_sentinels()


def test_a_captured_replay_equals_the_eager_bits():
    cameras = _cameras("three")
    eager = Bufs(3)
    eager.views(eager.cams(cameras))
    graph = Bufs(3)
    cams = graph.cams(cameras)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                          # (the capturing stream is the current one inside)
        graph.views(cams)
    torch.cuda.synchronize()
    assert bool((graph._g_idx == SENTINEL).all()), "the capture itself ran the kernels"
    g.replay()
    torch.cuda.synchronize()
    graph.check_sentinels()
    for name, got in graph.outputs().items():
        assert _bits(got, eager.outputs()[name]), name
