"""sln_layout_overlap_penalty on the device against the float64 restatement (evaluate.overlap_penalty_torch, held to central differences
by tests/test_overlap_penalty_host.py).  Gradients: per tensor |got - ref64| <= 2^-23 * max|ref64| + 8 * max|ref32 - ref64| with ref32
the float32 run of the restatement (the allowance form of tests/test_spade_leaf_gpu.py; the host test caps ref32's distance at 1e-4).
The penalty: 1e-12 relative against evaluate.layout_overlap's vol on the same mask - fp64 sums of the same float32 terms in another order.
Every comparison prints its figure before it asserts."""
import pytest
import torch

from conftest import pkg

import overlap_penalty_cases as OC

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 64                                   # sentinel elements on either side of every output
EV = pkg("host.evaluate")


def _device(c):
    rid, n_rooms = EV._room_ids(c["room_of_row"])
    return dict(b=c["boxes"].to(DEV), a=c["angles"].to(DEV), rr=c["room_of_row"].to(DEV), col=c["collide"].to(DEV), rid=rid.to(DEV), n_rooms=n_rooms)


def _guarded(shape, dtype, fill=None):
    """a tensor of ``shape`` inside a buffer with PAD sentinels on either side -> (view, check())"""
    n = 1
    for v in shape:
        n *= v
    sent = -12345.0
    buf = torch.full((n + 2 * PAD,), sent, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return view, lambda: bool((buf[:PAD] == sent).all()) and bool((buf[PAD + n:] == sent).all())


def _launch(d, weight=1.0, accumulate=False, onto=None):
    S, O, _ = d["b"].shape
    pen, ok_p = _guarded((S, d["n_rooms"]), torch.float64)
    gb, ok_b = _guarded((S, O, 6), torch.float32, None if onto is None else onto[0])
    ga, ok_a = _guarded((S, O), torch.float32, None if onto is None else onto[1])
    EV.overlap_penalty_launch(d["b"], d["a"], d["rr"], d["col"], d["rid"], d["n_rooms"], weight, accumulate, pen, gb, ga)
    torch.cuda.synchronize()
    assert ok_p() and ok_b() and ok_a(), "a write beside an output"
    return pen, gb, ga


def _references(c):
    args = (c["boxes"], c["angles"], c["room_of_row"], c["collide"])
    return EV.overlap_penalty_torch(*args), EV.overlap_penalty_torch(*args, dtype=torch.float32)


@pytest.mark.parametrize("name", OC.COMPARED)
def test_kernel_against_the_definition(name):
    c = OC.CASES[name]
    d = _device(c)
    pen, gb, ga = _launch(d)
    ref64, ref32 = _references(c)
    for what, got, r64, r32 in (("grad_boxes", gb, ref64[1], ref32[1]), ("grad_angles", ga, ref64[2], ref32[2])):
        scale = r64.abs().max().item()
        allowed = 2.0 ** -23 * scale + 8 * (r32.double() - r64).abs().max().item()
        err = (got.cpu().double() - r64).abs().max().item()
        print("%s %s: err %.3e, allowed %.3e (ratio %.3f), scale %.3e" % (name, what, err, allowed, err / allowed, scale))
        assert scale > 0 and err <= allowed
    vol, _ = EV.layout_overlap(d["b"], d["a"], d["rr"], d["col"])
    err = (pen.sum(1) - vol).abs().max().item()
    print("%s penalty %s, layout_overlap %s: err %.3e" % (name, pen.cpu().tolist(), vol.cpu().tolist(), err))
    assert (vol > 0).all() and err <= 1e-12 * vol.abs().max().item()
    per_room = ref64[0]
    assert (pen.cpu() - per_room).abs().max().item() <= 1e-5 * per_room.abs().max().item()     # (which room gets what: float32 terms against float64)
    # exact zeros: room rows and rows that do not collide
    O = c["boxes"].shape[1]
    quiet = ((c["room_of_row"].long() == torch.arange(O)) | (c["collide"] == 0)).to(DEV)
    assert quiet.any() and not gb[:, quiet].any() and not ga[:, quiet].any()


def test_disjoint_furniture_gives_exact_zeros():
    pen, gb, ga = _launch(_device(OC.CASES["g_disjoint"]))
    assert not pen.any() and not gb.any() and not ga.any()


@pytest.mark.parametrize("name", OC.FINITE_ONLY)
def test_degenerate_input_stays_finite(name):
    pen, gb, ga = _launch(_device(OC.CASES[name]))
    assert torch.isfinite(pen).all() and torch.isfinite(gb).all() and torch.isfinite(ga).all()


def test_nan_stays_in_its_room():
    c = OC.CASES["c_two_rooms"]
    d = _device(c)
    want = _launch(d)
    d["b"] = d["b"].clone()
    d["b"][0, 1, 0] = float("nan")
    d["a"] = d["a"].clone()
    d["a"][0, 2] = float("nan")
    pen, gb, ga = _launch(d)
    assert torch.equal(pen[:, 1], want[0][:, 1]) and torch.equal(gb[:, 4:], want[1][:, 4:]) and torch.equal(ga[:, 4:], want[2][:, 4:])


@pytest.mark.parametrize("name", ["c_two_rooms", "d_three_layouts", "e_many_rows"])
def test_accumulate_weight_and_repeatability(name):
    d = _device(OC.CASES[name])
    pen, gb, ga = _launch(d)
    again = _launch(d)
    assert torch.equal(pen, again[0]) and torch.equal(gb, again[1]) and torch.equal(ga, again[2])          # two calls: equal bits
    g = torch.Generator(device=DEV).manual_seed(7)
    xb, xa = torch.randn(gb.shape, generator=g, device=DEV), torch.randn(ga.shape, generator=g, device=DEV)
    pen1, gb1, ga1 = _launch(d, accumulate=True, onto=(xb, xa))
    assert torch.equal(pen1, pen) and torch.equal(gb1, xb + gb) and torch.equal(ga1, xa + ga)               # one float32 add per element
    pen0, gb0, ga0 = _launch(d, weight=0.0)
    assert torch.equal(pen0, pen) and not gb0.any() and not ga0.any()                                       # the penalty is unweighted
    penw, gbw, gaw = _launch(d, weight=0.25)
    assert torch.equal(penw, pen) and torch.equal(gbw, 0.25 * gb) and torch.equal(gaw, 0.25 * ga)           # (a power of two: exact)


def test_layouts_of_a_batch_are_independent():
    """S > 1: layout s of the batch has the bits of layout s alone (several layouts per workgroup; a batch that fills more than one)"""
    c = OC.CASES["d_three_layouts"]
    d = _device(c)
    many = dict(d, b=d["b"].repeat(23, 1, 1), a=d["a"].repeat(23, 1))                  # 69 layouts of 5 rows: several per workgroup, nine workgroups
    pen, gb, ga = _launch(many)
    for s in range(3):
        one = dict(d, b=d["b"][s:s + 1].contiguous(), a=d["a"][s:s + 1].contiguous())
        p1, b1, a1 = _launch(one)
        for k in (s, s + 33, s + 66):
            assert torch.equal(pen[k], p1[0]) and torch.equal(gb[k], b1[0]) and torch.equal(ga[k], a1[0])


def test_rooms_of_a_long_layout_are_independent():
    """one layout of 60 rooms (4 and 5 rows in turn, 270 rows: several tiles dealt to several workgroups, rows in passes): every room has
    the bits of the room alone; the second layout of the batch is a jittered one"""
    three, four = OC._room(OC.FURNITURE[:3]), OC._room(OC.FURNITURE)
    c = OC._case([three, four] * 30, S=2, jitter=0.05, seed=11)
    pen, gb, ga = _launch(_device(c))
    assert (pen > 0).all() and pen.shape == (2, 60)
    a = 0
    for r in range(60):
        n = 4 + r % 2
        one = dict(boxes=c["boxes"][:, a:a + n].contiguous(), angles=c["angles"][:, a:a + n].contiguous(),
                   room_of_row=torch.full((n,), n - 1, dtype=torch.int32), collide=c["collide"][a:a + n])
        p1, b1, a1 = _launch(_device(one))
        assert torch.equal(pen[:, r], p1[:, 0]) and torch.equal(gb[:, a:a + n], b1) and torch.equal(ga[:, a:a + n], a1), r
        a += n


def test_a_room_beyond_the_tile_cap():
    """a room of more than MAX_ROOM_ROWS rows (the host entry points refuse it): NaN penalty and zero gradients, the room in front of
    it as ever; with accumulate = 1 what is there stays"""
    n = EV.MAX_ROOM_ROWS + 6
    small = OC.CASES["a_generic"]
    g = torch.Generator().manual_seed(2)
    lo = torch.rand(n, 3, generator=g) * 0.5
    big = torch.cat([lo, lo + 0.3], 1)
    big[-1] = torch.tensor([0.0, 0.0, 0.0, 6.0, 3.0, 5.0])
    c = dict(boxes=torch.cat([small["boxes"][0], big])[None].contiguous(), angles=torch.cat([small["angles"][0], torch.zeros(n)])[None].contiguous(),
             room_of_row=torch.cat([small["room_of_row"], torch.full((n,), 5 + n - 1, dtype=torch.int32)]),
             collide=torch.cat([small["collide"], torch.ones(n, dtype=torch.uint8)]))
    d = dict(b=c["boxes"].to(DEV), a=c["angles"].to(DEV), rr=c["room_of_row"].to(DEV), col=c["collide"].to(DEV),
             rid=torch.cat([torch.zeros(5, dtype=torch.int32), torch.ones(n, dtype=torch.int32)]).to(DEV), n_rooms=2)
    pen, gb, ga = _launch(d)
    p1, b1, a1 = _launch(_device(small))
    assert torch.equal(pen[:, 0], p1[:, 0]) and bool(torch.isnan(pen[:, 1]).all())
    assert torch.equal(gb[:, :5], b1) and torch.equal(ga[:, :5], a1) and not gb[:, 5:].any() and not ga[:, 5:].any()
    xb, xa = torch.full_like(gb, 3.0), torch.full_like(ga, -2.0)
    _, gb2, ga2 = _launch(d, accumulate=True, onto=(xb, xa))
    assert torch.equal(gb2[:, :5], 3.0 + b1) and bool((gb2[:, 5:] == 3.0).all()) and bool((ga2[:, 5:] == -2.0).all())


def test_badarg():
    L = pkg("_lib")
    d = _device(OC.CASES["a_generic"])
    S, O, _ = d["b"].shape
    pen = torch.full((S, 1), -7.0, dtype=torch.float64, device=DEV)
    gb, ga = torch.full((S, O, 6), -7.0, device=DEV), torch.full((S, O), -7.0, device=DEV)
    lib, P, st = L.lib(), L.ptr, L.current_stream_ptr()
    good = [P(d["b"]), P(d["a"]), P(d["rr"]), P(d["col"]), P(d["rid"]), 1, S, O, 1.0, 0, P(pen), P(gb), P(ga), st]
    for k in (0, 1, 2, 3, 4, 10, 11, 12):                                              # a null pointer
        assert lib.sln_layout_overlap_penalty(*(good[:k] + [None] + good[k + 1:])) == -1
    for k, v in ((5, 0), (6, -1), (7, -1), (8, -1.0), (8, float("nan")), (9, 2), (9, -1)):
        assert lib.sln_layout_overlap_penalty(*(good[:k] + [v] + good[k + 1:])) == -1
    assert lib.sln_layout_overlap_penalty(*(good[:6] + [0] + good[7:])) == 0           # S = 0: nothing to do
    torch.cuda.synchronize()
    assert bool((pen == -7).all()) and bool((gb == -7).all()) and bool((ga == -7).all())   # refused before any launch
    assert lib.sln_layout_overlap_penalty(*good) == 0
    torch.cuda.synchronize()
    assert bool((pen != -7).all()) and bool((gb != -7).all())


def test_autograd_function_scales_rows_by_their_room():
    c = OC.CASES["c_two_rooms"]
    d = _device(c)
    _, gb, ga = _launch(d)
    b, a = d["b"].clone().requires_grad_(True), d["a"].clone().requires_grad_(True)
    pen = EV.overlap_penalty(b, a, d["rr"], d["col"])
    up = torch.tensor([[1.0, 0.5]], dtype=torch.float64, device=DEV)
    (pen * up).sum().backward()
    assert pen.dtype == torch.float64 and pen.shape == (1, 2)
    assert torch.equal(b.grad[:, :4], gb[:, :4]) and torch.equal(a.grad[:, :4], ga[:, :4])                  # room 0: untouched
    assert torch.equal(b.grad[:, 4:], 0.5 * gb[:, 4:]) and torch.equal(a.grad[:, 4:], 0.5 * ga[:, 4:])      # room 1: halved
    assert gb[:, :4].abs().sum() > 0 and gb[:, 4:].abs().sum() > 0
