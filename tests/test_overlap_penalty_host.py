"""The definition of the interpenetration penalty on the CPU: ``evaluate.overlap_penalty_torch`` against central differences of
``layout_overlap_torch``, its value, its exact zeros, the tie rule of the height factor, degenerate input, descent, the float32 run
against the float64 run (the cap that keeps the GPU test's allowance from hiding a failure) and the refusals of the host entry points.
Every comparison prints its figure before it asserts."""
import pytest
import torch

from conftest import pkg

import overlap_penalty_cases as OC

EV = pkg("host.evaluate")
FD_H = 1e-6
FD_BOUND = 1e-6            # of the layout's largest gradient entry: the ring part measures ~1e-8, FD rounding is ~2e-10 / h
VALUE_BOUND = 1e-12
F32_BOUND = 1e-4           # float32 run against float64 run, of the tensor's largest entry


def _run(name, dtype=torch.float64):
    c = OC.CASES[name]
    return c, EV.overlap_penalty_torch(c["boxes"], c["angles"], c["room_of_row"], c["collide"], dtype=dtype)


def _central_differences(c):
    """d layout_overlap_torch(...)[0] / d (box[0:6], angle) of every row of every layout by central differences in float64: all the
    perturbed layouts of one layout go through ONE call"""
    b, a = c["boxes"].double(), c["angles"].double()
    S, O, _ = b.shape
    out = torch.zeros(S, O, 7, dtype=torch.float64)
    for s in range(S):
        x = torch.cat([b[s], a[s][:, None]], 1).flatten()                               # [O * 7]
        n = x.numel()
        both = torch.cat([x[None] + FD_H * torch.eye(n, dtype=torch.float64), x[None] - FD_H * torch.eye(n, dtype=torch.float64)]).reshape(2 * n, O, 7)
        vol = EV.layout_overlap_torch(both[..., :6], both[..., 6], c["room_of_row"], c["collide"])[0]
        out[s] = ((vol[:n] - vol[n:]) / (2 * FD_H)).reshape(O, 7)
    return out


@pytest.mark.parametrize("name", OC.FD_CASES)
def test_gradient_against_central_differences(name):
    c, (pen, gb, ga) = _run(name)
    fd = _central_differences(c)
    got = torch.cat([gb, ga[..., None]], -1)
    furniture = c["room_of_row"].long() != torch.arange(c["boxes"].shape[1])           # (a room row moves the extent: a constant here)
    for s in range(got.shape[0]):
        scale = got[s].abs().max().item()
        err = (got[s] - fd[s])[furniture].abs().max().item()
        print("%s layout %d: |grad - fd| %.3e of max|grad| %.3e = %.3e (bound %.0e)" % (name, s, err, scale, err / scale, FD_BOUND))
        assert scale > 0
        assert err <= FD_BOUND * scale


@pytest.mark.parametrize("name", list(OC.CASES))
def test_value_is_layout_overlap(name):
    c, (pen, _, _) = _run(name)
    vol = EV.layout_overlap_torch(c["boxes"], c["angles"], c["room_of_row"], c["collide"])[0]
    err = (pen.sum(1) - vol).abs().max().item()
    print("%s: penalty %s, vol %s, err %.3e" % (name, pen.tolist(), vol.tolist(), err))
    assert pen.dtype == torch.float64 and pen.shape == (c["boxes"].shape[0], int(c["room_of_row"].unique().numel()))
    assert err <= VALUE_BOUND * vol.abs().max().item()
    if name in OC.COMPARED:
        assert (vol > 0).all()


def test_pairs_across_rooms_do_not_count():
    c, (pen, gb, ga) = _run("c_two_rooms")
    one_room = dict(c, room_of_row=torch.full_like(c["room_of_row"], c["boxes"].shape[1] - 1))
    both = EV.layout_overlap_torch(c["boxes"], c["angles"], one_room["room_of_row"], c["collide"])[0]
    print("two rooms %s, as one room %s" % (pen.tolist(), both.tolist()))
    assert (pen > 0).all() and both.item() > pen.sum().item() * 1.01                   # (the pairs across the boundary WOULD overlap)
    first = OC.CASES["a_generic"]                                                      # room 1 of (c) is (a): same numbers
    pa, gba, gaa = EV.overlap_penalty_torch(first["boxes"], first["angles"], first["room_of_row"], first["collide"])
    assert torch.equal(pen[:, 1], pa[:, 0]) and torch.equal(gb[:, 4:], gba) and torch.equal(ga[:, 4:], gaa)


def test_exact_zeros():
    _, (pen, gb, ga) = _run("g_disjoint")
    assert torch.equal(pen, torch.zeros_like(pen)) and not gb.any() and not ga.any()
    for name in OC.COMPARED:
        c, (pen, gb, ga) = _run(name)
        O = c["boxes"].shape[1]
        quiet = (c["room_of_row"].long() == torch.arange(O)) | (c["collide"] == 0)
        assert quiet.any() and not gb[:, quiet].any() and not ga[:, quiet].any(), name
        assert gb[:, ~quiet].abs().sum() > 0, name


def test_room_row_that_collides_keeps_a_zero_gradient():
    c = OC.CASES["a_generic"]
    every = torch.ones_like(c["collide"])
    pen, gb, ga = EV.overlap_penalty_torch(c["boxes"], c["angles"], c["room_of_row"], every)
    assert pen.item() > _run("a_generic")[1][0].item() and not gb[:, -1].any() and not ga[:, -1].any()


def test_height_ties_split_in_halves():
    """the height factor alone against the autograd of torch.minimum / torch.maximum / clamp: floor-standing furniture ties at h0 = 0,
    rows 0 and 1 tie at h1, row 3 stands on row 2 (overlap exactly 0: nothing)"""
    c, (pen, gb, ga) = _run("h_height_ties")
    b = c["boxes"].double()
    _, h0, h1 = EV.cuboids_torch(b, c["angles"].double(), c["room_of_row"])
    assert (h0[0, :3] == 0).all() and h1[0, 0] == h1[0, 1] and h0[0, 3] == h1[0, 2]
    ring = EV.cuboids_torch(b, c["angles"].double(), c["room_of_row"])[0]
    i, j = torch.triu_indices(4, 4, 1)
    area = EV.quad_intersection_area_torch(ring[0, i], ring[0, j])
    assert (area > 0).all()
    y = b[0, :4][:, [1, 4]].clone().requires_grad_(True)                                # (y0, y1) of the furniture, in room units
    ext_y = b[0, -1, 4]
    lo, hi = y[:, 0] * ext_y, y[:, 1] * ext_y
    hov = (torch.minimum(hi[i], hi[j]) - torch.maximum(lo[i], lo[j]))
    (area * torch.where(hov > 0, hov, torch.zeros_like(hov))).sum().backward()
    err = (gb[0, :4][:, [1, 4]] - y.grad).abs().max().item()
    print("height gradients %s against autograd %s: err %.3e" % (gb[0, :4][:, [1, 4]].tolist(), y.grad.tolist(), err))
    assert err <= 1e-12 * y.grad.abs().max().item()
    stacked = EV.overlap_penalty_torch(c["boxes"][:, [2, 3, 4]], c["angles"][:, [2, 3, 4]], torch.tensor([2, 2, 2], dtype=torch.int32), c["collide"][[2, 3, 4]])
    assert not stacked[0].any() and not stacked[1].any() and not stacked[2].any()      # a height overlap of 0: nothing at all


@pytest.mark.parametrize("name", OC.FINITE_ONLY)
def test_degenerate_input_stays_finite(name):
    for dtype in (torch.float64, torch.float32):
        _, out = _run(name, dtype)
        assert all(torch.isfinite(t).all() for t in out), name


def test_nan_stays_in_its_room():
    c = OC.CASES["c_two_rooms"]
    b = c["boxes"].clone()
    b[0, 1, 0] = float("nan")
    pen, gb, ga = EV.overlap_penalty_torch(b, c["angles"], c["room_of_row"], c["collide"])
    _, (p0, gb0, ga0) = _run("c_two_rooms")
    assert torch.equal(pen[:, 1], p0[:, 1]) and torch.equal(gb[:, 4:], gb0[:, 4:]) and torch.equal(ga[:, 4:], ga0[:, 4:])


def test_descent():
    c, (pen, gb, ga) = _run("a_generic")
    eps = 1e-3 / max(gb.abs().max().item(), ga.abs().max().item())
    after = EV.overlap_penalty_torch(c["boxes"].double() - eps * gb, c["angles"].double() - eps * ga, c["room_of_row"], c["collide"])[0]
    print("penalty %.9f -> %.9f" % (pen.item(), after.item()))
    assert after.item() < pen.item()


@pytest.mark.parametrize("name", OC.COMPARED)
def test_float32_run_stays_close_to_float64(name):
    _, ref = _run(name)
    _, low = _run(name, torch.float32)
    for what, r, l in zip(("penalty", "grad_boxes", "grad_angles"), ref, low):
        assert l.dtype == torch.float32
        err, scale = (l.double() - r).abs().max().item(), r.abs().max().item()
        print("%s %s: |f32 - f64| %.3e of %.3e = %.3e (bound %.0e)" % (name, what, err, scale, err / scale, F32_BOUND))
        assert err <= F32_BOUND * scale


def test_autograd_function_on_cpu_tensors():
    c = OC.CASES["c_two_rooms"]
    b, a = c["boxes"].clone().requires_grad_(True), c["angles"].clone().requires_grad_(True)
    pen = EV.overlap_penalty(b, a, c["room_of_row"], c["collide"])
    up = torch.tensor([[2.0, -0.5]], dtype=torch.float64)
    (pen * up).sum().backward()
    _, (p0, gb, ga) = _run("c_two_rooms")
    scale = torch.tensor([2.0] * 4 + [-0.5] * 5, dtype=torch.float64)
    assert torch.equal(pen.detach(), p0) and b.grad.dtype == torch.float32
    assert torch.equal(b.grad, (gb * scale[None, :, None]).float()) and torch.equal(a.grad, (ga * scale[None]).float())


def test_collide_rows():
    names = ["bed", "wall", "__room__", "lamp", "window"]
    objs = torch.tensor([0, 1, 3, 2, 4, 0, 2])
    got = EV.collide_rows(objs, names, 2)
    assert got.tolist() == [True, False, True, False, False, True, False]
    assert EV.visible_rows(objs, names).tolist()[3] is True                             # (visible_rows keeps the room rows)


def test_refine_argument_check():
    R = pkg("host.refine")
    rooms = [(3, ["bed", "wall", "__room__"]), (2, ["lamp", "__room__"])]
    assert R.check_overlap(0.0, None, rooms) is None and R.check_overlap(0.0, None, [(3, ["bed"])]) is None
    assert R.check_overlap(0.5, None, rooms) == [[True, False, False], [True, False]]
    assert R.check_overlap(0.5, [None, (False, True)], rooms) == [[True, False, False], [False, False]]        # (a room row never collides)
    assert R.check_overlap(0.5, [[True, True, False], None], [(3, ["bed"]), rooms[1]])[0] == [True, True, False]
    for bad in (-1e-3, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="overlap_weight"):
            R.check_overlap(bad, None, rooms)
    with pytest.raises(ValueError, match="class_names"):
        R.check_overlap(0.5, None, [(3, ["bed"])])
    with pytest.raises(ValueError, match="overlap_rows"):
        R.check_overlap(0.5, [None], rooms)
    with pytest.raises(ValueError, match="overlap_rows"):
        R.check_overlap(0.5, [[True], None], rooms)
    n = EV.MAX_ROOM_ROWS + 1
    with pytest.raises(ValueError, match="more than"):
        R.check_overlap(0.5, None, [(n, ["bed"] * n)])
    assert R.check_overlap(0.0, None, [(n, ["bed"] * n)]) is None


def test_loops_refuse_in_front_of_their_first_launch_and_the_cpu_term_is_the_restatement():
    import types
    R = pkg("host.refine")
    # a stand-in model and rooms without tensors a launch would need: the refusals come first
    model = types.SimpleNamespace(flat_params=torch.zeros(1))
    rooms = [dict(objs=torch.zeros(3, dtype=torch.int64), class_names=["bed", "lamp", "__room__"])] * 2
    for kw in (dict(overlap_weight=-1.0), dict(overlap_weight=float("nan")), dict(overlap_weight=1.0, overlap_rows=[[True, False, False]]),
               dict(overlap_weight=1.0, overlap_rows=[[True], None])):
        with pytest.raises(ValueError, match="overlap"):
            R.RefineBatch(model, rooms, image_size=16, **kw)
    with pytest.raises(ValueError, match="class_names"):
        R.RefineBatch(model, [dict(rooms[0], class_names=["bed"])], image_size=16, overlap_weight=1.0)
    args = (None, None, None, torch.zeros(3, 6), None, None, ["bed", "lamp", "__room__"])
    for loop in (R.finetune_vae, R.finetune_vae_fast):
        with pytest.raises(ValueError, match="overlap_weight"):
            loop(*args, image_size=16, overlap_weight=-2.0)
        with pytest.raises(ValueError, match="overlap_rows"):
            loop(*args, image_size=16, overlap_weight=1.0, overlap_rows=[True, False])
    # the term the one-room loops add, on CPU tensors: weight * the restatement, float32, followed by autograd
    c = OC.CASES["a_generic"]
    names = ["bed", "lamp", "wall", "desk", "__room__"]
    tables = R._one_room_overlap(0.5, None, names, 5, "cpu")
    assert tables[0].tolist() == [1, 1, 0, 1, 0] and tables[1].tolist() == [4] * 5 and tables[2].tolist() == [0] * 5
    assert R._one_room_overlap(0.0, None, names, 5, "cpu") is None
    b, a = c["boxes"][0].clone().requires_grad_(True), c["angles"][0].clone().requires_grad_(True)
    term = R._overlap_term(b, a, tables, 0.5)
    term.backward()
    pen, gb, ga = EV.overlap_penalty_torch(c["boxes"], c["angles"], c["room_of_row"], tables[0])
    assert term.dtype == torch.float32 and term.item() == (pen * 0.5).float().item() and pen.item() > 0
    assert torch.equal(b.grad, (0.5 * gb[0]).float()) and torch.equal(a.grad, (0.5 * ga[0]).float()) and not b.grad[2].any()


def test_refusals():
    c = OC.CASES["a_generic"]
    b, a, rr, col = c["boxes"], c["angles"], c["room_of_row"], c["collide"]
    for fn in (EV.overlap_penalty, EV.overlap_penalty_torch):
        with pytest.raises(ValueError):
            fn(b[0], a, rr, col)                                                         # not [S, O, 6]
        with pytest.raises(ValueError):
            fn(b, a[:, :-1], rr, col)
        with pytest.raises(ValueError):
            fn(b, a, rr, col[:-1])
        with pytest.raises(ValueError):
            fn(b, a, torch.zeros_like(rr), col)                                          # a table that names rows in front of a row
    n = EV.MAX_ROOM_ROWS + 1
    with pytest.raises(ValueError, match="more than"):
        EV.overlap_penalty(torch.zeros(1, n, 6), torch.zeros(1, n), torch.full((n,), n - 1, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8))
