"""Host logic of the ONE wgrad launch of a full iteration (csrc/gemm_f32.hip::sln_tn_mixed_plan) - runs without a GPU: every
(problem, output tile, row chunk) of the whole list appears exactly once and carries its problem's gather bit, all tiles of one
(problem, chunk) sit on ONE XCD in consecutive slots, the XCDs' loads are balanced, the chunks are the ones the per-kind planner
gives the same problems (so a problem's per-element sums do not depend on the route), and a list that does not fit the table at
that chunk length is refused instead of given longer chunks."""
import ctypes as C

import numpy as np

from conftest import pkg
from test_tn_plan import _plan as _plan_per_kind

MAX_ITEMS = 16384


def _plan(shapes, gathers):
    lib = pkg("_lib").lib()
    R, N, K = (np.ascontiguousarray([s[i] for s in shapes], np.int32) for i in range(3))
    g = np.ascontiguousarray(gathers, np.int32)
    rpb = np.zeros(len(shapes), np.int32)
    items = np.full((MAX_ITEMS, 4), -7, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nb = lib.sln_debug_tn_plan_mixed(p(R), p(N), p(K), p(g), len(shapes), p(rpb), p(items), MAX_ITEMS)
    return nb, rpb, items[:max(nb, 0)]


def _check(shapes, gathers, rpb, items):
    assert items.shape[0] % 8 == 0
    seen = {}
    for b, (p, t, c, xg) in enumerate(items):
        if p < 0:
            continue
        assert (p, t, c) not in seen, "duplicate work item"
        assert xg == (1 if gathers[p] else 0), "item %d carries the wrong gather bit" % b
        seen[(p, t, c)] = b
    want = 0
    per_xcd = np.zeros(8)
    for p, (R, N, K) in enumerate(shapes):
        assert rpb[p] % 32 == 0 and rpb[p] > 0
        tiles, chunks = -(-N // 64) * -(-K // 64), -(-R // rpb[p])
        want += tiles * chunks
        for c in range(chunks):
            slots = [seen[(p, t, c)] for t in range(tiles)]              # KeyError = a missing item
            assert len({s % 8 for s in slots}) == 1, "tiles of one (problem, chunk) on several XCDs"
            assert slots == list(range(slots[0], slots[0] + 8 * tiles, 8)), "tiles of a group are consecutive on their XCD"
            per_xcd[slots[0] % 8] += tiles * min(rpb[p], R - c * rpb[p])
    assert len(seen) == want
    return per_xcd


def _step_shapes(graphs):
    """Both passes of a step of the default model: per net 5 layers (net1.0 gathers) + heads."""
    T, O, H, D = 64 * graphs, 32 * graphs, 256, 128
    shapes, gathers = [], []
    for _ in range(2):
        for _ in range(5):
            shapes += [(T, H, 3 * D), (T, 2 * H + D, H), (O, H, H), (O, D, H)]
            gathers += [1, 0, 0, 0]
        shapes += [(O, H, 128), (O, 128, H), (O, 48, 128), (O, 48, 128), (O, 16, 128), (O, 16, 128)]
        gathers += [0] * 6
    return shapes, gathers


def test_the_64_graph_step_is_covered_once_and_balanced():
    shapes, gathers = _step_shapes(64)
    nb, rpb, items = _plan(shapes, gathers)
    assert nb > 4096, "the whole step does not fit one per-kind table: %d workgroups" % nb
    load = _check(shapes, gathers, rpb, items)
    assert load.max() <= 1.15 * load.mean(), load                       # longest-first dealing keeps the XCDs within 15 %
    pad = int((items[:, 0] < 0).sum())
    assert pad <= 0.05 * nb, "%d of %d workgroups are padding" % (pad, nb)


def test_chunks_are_the_per_kind_planner_s():
    shapes, gathers = _step_shapes(64)
    nb, rpb, _ = _plan(shapes, gathers)
    assert nb > 0
    for kind in (0, 1):
        sel = [i for i, g in enumerate(gathers) if g == kind]
        rpb_kind, _ = _plan_per_kind([shapes[i] for i in sel])
        assert list(rpb_kind) == [rpb[i] for i in sel]


def test_ragged_shapes_128_problems():
    base = [(13, 8, 36), (100, 24, 256), (4097, 640, 256), (33, 70, 130), (2048, 6, 256), (1, 130, 6), (705, 96, 96), (31, 6, 6)]
    shapes = [base[i % len(base)] for i in range(128)]
    gathers = [(i * 7) % 3 == 0 for i in range(128)]
    nb, rpb, items = _plan(shapes, gathers)
    assert nb > 0
    _check(shapes, gathers, rpb, items)
    assert _plan(shapes + [base[0]], gathers + [0])[0] == -1          # 129 problems


def test_a_list_past_the_table_is_refused_not_given_longer_chunks():
    shapes, gathers = _step_shapes(512)
    assert _plan(shapes, gathers)[0] == -1
    shapes, gathers = _step_shapes(128)                                 # the largest step of the default model that still fits
    nb, rpb, items = _plan(shapes, gathers)
    assert 0 < nb <= MAX_ITEMS
    _check(shapes, gathers, rpb, items)
    assert max(rpb) <= 768


def test_deterministic_mode_plans_one_chunk_per_problem():
    lib = pkg("_lib").lib()
    shapes, gathers = [(4096, 640, 256), (2048, 256, 256), (4096, 256, 384)], [0, 0, 1]
    try:
        lib.sln_set_deterministic(1)
        nb, rpb, items = _plan(shapes, gathers)
    finally:
        lib.sln_set_deterministic(0)
    assert nb > 0
    _check(shapes, gathers, rpb, items)
    assert {c for p, t, c, _ in items if p >= 0} == {0}
