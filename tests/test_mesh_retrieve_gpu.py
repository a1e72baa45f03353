"""Mesh retrieval on the device (csrc/mesh_retrieve.hip through host/retrieve.py): the kernels against the choices of the reference's own
functions (tests/golden/mesh_retrieve.npz) and against the torch restatement, evaluated on the host, at the shapes where the indexing
can break.  The output is an argmin: every comparison is for equality."""
import numpy as np
import pytest
import torch

from conftest import pkg
from gpu_util import _lib, _sync
from test_mesh_retrieve_host import golden_tables

pytestmark = pytest.mark.gpu

CHUNK = 2048                # models per LDS chunk (csrc/mesh_retrieve.hip: RT_CHUNK)


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int64), b.cpu().contiguous().view(torch.int64))


def test_kernel_equals_the_reference_choice_and_the_float64_restatement():
    _lib()
    RT = pkg("host.retrieve")
    g, vocab, data, wall = golden_tables()
    table = RT.ModelTable(data, vocab, "cuda")
    boxes, objs, room_row = torch.from_numpy(g["boxes"]), torch.from_numpy(g["objs"]), torch.from_numpy(g["room_row"])
    choice, dist = RT.retrieve_models(boxes.cuda(), objs.cuda(), room_row.cuda(), table, dist=True)
    _sync("sln_mesh_retrieve")
    assert choice.dtype == torch.int32 and choice.shape == (boxes.shape[0],)
    assert int((choice.cpu().numpy() != g["choice"]).sum()) == 0
    want, want_d = RT.retrieve_models_torch(boxes, objs, room_row, RT.ModelTable(data, vocab), dist=True)
    assert torch.equal(choice.cpu(), want)
    same = (dist.cpu() == want_d) | (torch.isnan(dist.cpu()) & torch.isnan(want_d))
    assert bool(same.all()) and _same_bits(torch.nan_to_num(dist, nan=-1.0), torch.nan_to_num(want_d, nan=-1.0))
    # without the optional output, the same choice
    assert torch.equal(RT.retrieve_models(boxes.cuda(), objs.cuda(), room_row.cuda(), table), choice)
    _sync("sln_mesh_retrieve without dist")


def test_nan_rule_and_all_infinite_rows():
    """The zero-width room of the fixture: a zero-width slab box against the zero-width slab models (inf - inf: the FIRST NaN, model 2, beats
    the finite and infinite distances in front of it), a zero-width chair box (every distance infinite: index 0, distance inf), boxes of
    zero width and height (0 / 0: every distance NaN, index 0)."""
    _lib()
    RT = pkg("host.retrieve")
    g, vocab, data, wall = golden_tables()
    table = RT.ModelTable(data, vocab, "cuda")
    rr = g["room_row"]
    ext = g["boxes"][rr][:, 3]
    zero_w = (g["boxes"][:, 3] * ext - g["boxes"][:, 0] * ext == 0) & (rr != np.arange(len(rr)))
    rows = np.nonzero(zero_w)[0]
    assert len(rows) == 5
    choice, dist = RT.retrieve_models(torch.from_numpy(g["boxes"]).cuda(), torch.from_numpy(g["objs"]).cuda(), torch.from_numpy(rr).cuda(), table, dist=True)
    _sync("sln_mesh_retrieve")
    choice, dist = choice.cpu().numpy(), dist.cpu().numpy()
    assert (choice[rows] == g["choice"][rows]).all()
    got = sorted((vocab[g["objs"][i]], int(choice[i]), "nan" if np.isnan(dist[i]) else str(dist[i])) for i in rows)
    assert got == sorted([("slab", 2, "nan"), ("slab", 2, "nan"), ("slab", 0, "nan"), ("chair", 0, "inf"), ("chair", 0, "nan")]), got


def _random_case(N, S, seed):
    rng = np.random.default_rng(seed)
    lens = [N] if N < 3 else [N // 2 + 1, N // 3, N - (N // 2 + 1) - N // 3]
    lens = [n for n in lens if n > 0]
    assert sum(lens) == N
    last = np.cumsum(lens) - 1
    room_row = np.repeat(last, lens).astype(np.int32)
    is_room = room_row == np.arange(N)
    objs = rng.choice([1, 2, 3, 4, 7, -1], size=N, p=[0.15, 0.55, 0.05, 0.15, 0.05, 0.05]).astype(np.int32)      # 7, -1: outside the table
    objs[is_room] = 0
    lo = rng.uniform(0.0, 0.6, size=(S, N, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(0.05, 0.4, size=(S, N, 3))], 2).astype(np.float32)
    boxes[:, is_room] = np.concatenate([np.zeros((S, int(is_room.sum()), 3)), rng.uniform(2.5, 7.0, size=(S, int(is_room.sum()), 3))], 2).astype(np.float32)
    # class 2 has more models than one chunk and starts at table row 5: its slice [5, 2505) spans two chunks
    big = 2500

    def entry(k, size):
        return {"id": "m%d" % k, "bbox_min": [0.0, 0.0, 0.0], "bbox_max": [float(x) for x in size]}
    data = {"a": [entry(k, s) for k, s in enumerate(rng.uniform(0.3, 2.0, size=(5, 3)))],
            "big": [entry(k, s) for k, s in enumerate(rng.uniform(0.3, 2.0, size=(big, 3)))], "none": [],
            "d": [entry(k, s) for k, s in enumerate(rng.uniform(0.3, 2.0, size=(40, 3)))]}
    planted = {}
    rows_big = np.nonzero(objs == 2)[0]
    if len(rows_big) >= 2:
        # the ratios of two query rows (layout 0), planted as table entries with x size 1 and bbox_min 0: distance exactly 0
        with np.errstate(all="ignore"):
            ext = boxes[0][room_row][:, 3:]
            d = boxes[0][:, 3:] * ext - boxes[0][:, :3] * ext
            ratio = np.stack([d[:, 1] / d[:, 0], d[:, 2] / d[:, 0]], 1).astype(np.float64)
        i, j = int(rows_big[0]), int(rows_big[-1])
        assert 5 + 2400 >= CHUNK and 5 + 17 < CHUNK
        data["big"][2400] = entry(2400, (1.0, ratio[i, 0], ratio[i, 1]))      # the minimum in the last chunk ...
        data["big"][17] = entry(17, (1.0, ratio[i, 0], ratio[i, 1]))          # ... and its duplicate in the first: the first wins
        data["big"][2450] = entry(2450, (1.0, ratio[j, 0], ratio[j, 1]))      # a minimum that only the last chunk holds
        planted = {i: 17, j: 2450}
    vocab = ["__room__", "a", "big", "none", "d"]
    return boxes, objs, room_row, data, vocab, planted


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 65, 257, 1025])
def test_kernel_equals_the_restatement_on_random_rooms(N, S):
    _lib()
    RT = pkg("host.retrieve")
    boxes, objs, room_row, data, vocab, planted = _random_case(N, S, seed=100 + N)
    host = RT.ModelTable(data, vocab)
    assert host.n_models > CHUNK and host.class_ptr_host[2] < CHUNK < host.class_ptr_host[3]
    want, want_d = RT.retrieve_models_torch(torch.from_numpy(boxes), torch.from_numpy(objs), torch.from_numpy(room_row), host, dist=True)
    b = torch.from_numpy(boxes if S > 1 else boxes[0]).cuda()
    choice, dist = RT.retrieve_models(b, torch.from_numpy(objs).cuda(), torch.from_numpy(room_row).cuda(), RT.ModelTable(data, vocab, "cuda"), dist=True)
    _sync("sln_mesh_retrieve N=%d S=%d" % (N, S))
    assert choice.shape == ((S, N) if S > 1 else (N,))
    choice, dist = choice.cpu().reshape(S, N), dist.cpu().reshape(S, N)
    assert torch.equal(choice, want), "%d rows differ" % int((choice != want).sum())
    assert _same_bits(torch.nan_to_num(dist, nan=-1.0), torch.nan_to_num(want_d, nan=-1.0)) and torch.equal(torch.isnan(dist), torch.isnan(want_d))
    is_room = torch.from_numpy(room_row == np.arange(N))
    outside = torch.from_numpy((objs < 0) | (objs >= len(vocab)) | (objs == 3))
    assert bool((choice[:, is_room | outside] == -1).all()) and bool((choice[:, ~(is_room | outside)] >= 0).all())
    if N >= 63:
        assert len(planted) == 2
    for row, k in planted.items():
        assert int(choice[0, row]) == k and float(dist[0, row]) == 0.0, (row, k, int(choice[0, row]))
    if N >= 257:
        assert int((choice[:, torch.from_numpy(objs == 2)] >= CHUNK - 5).sum()) > 1, "no row chose a model of the second chunk"


@pytest.mark.parametrize("R", [1, 5])
def test_shell_retrieval_equals_golden_and_restatement(R):
    _lib()
    RT = pkg("host.retrieve")
    g, vocab, data, wall = golden_tables()
    wr, fr = (torch.from_numpy(x) for x in RT.shell_ratios(wall))
    boxes = torch.from_numpy(g["boxes"])
    if R == 5:
        last = torch.from_numpy(g["last_row"])
        got = RT.retrieve_shell(boxes.cuda(), last.cuda(), wr.cuda(), fr.cuda())
        _sync("sln_shell_retrieve")
        assert got.dtype == torch.int32 and got.shape == (len(last), 2)
        assert torch.equal(got.cpu()[:, 0], torch.from_numpy(g["wall_choice"])) and torch.equal(got.cpu()[:, 1], torch.from_numpy(g["floor_choice"]))
    # R rooms of random extents, among them a degenerate one (X = 0: every distance infinite or NaN -> index 0 either way)
    rng = np.random.default_rng(R)
    rooms = np.zeros((R + 2, 6), dtype=np.float32)
    rooms[:, 3:] = rng.uniform(2.0, 8.0, size=(R + 2, 3))
    rooms[1, 3] = 0.0 if R == 5 else rooms[1, 3]
    last = torch.arange(1, R + 1, dtype=torch.int32).flip(0).contiguous()          # (any order, not every row)
    got = RT.retrieve_shell(torch.from_numpy(rooms).cuda(), last.cuda(), wr.cuda(), fr.cuda())
    _sync("sln_shell_retrieve R=%d" % R)
    assert torch.equal(got.cpu(), RT.retrieve_shell_torch(torch.from_numpy(rooms), last, wr, fr))
    empty = RT.retrieve_shell(torch.from_numpy(rooms).cuda(), last.cuda(), wr[:0].cuda(), fr[:0].cuda())
    _sync("sln_shell_retrieve W=0")
    assert bool((empty == -1).all())


def test_call_is_capturable_and_allocates_nothing():
    _lib()
    RT = pkg("host.retrieve")
    boxes, objs, room_row, data, vocab, _ = _random_case(257, 3, seed=9)
    table = RT.ModelTable(data, vocab, "cuda")
    b, o, rr = torch.from_numpy(boxes).cuda(), torch.from_numpy(objs).cuda(), torch.from_numpy(room_row).cuda()
    choice = torch.full((3, 257), -5, dtype=torch.int32, device="cuda")
    dist = torch.zeros(3, 257, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RT.into(b, o, rr, table, choice, dist)                           # warmed
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        RT.into(b, o, rr, table, choice, dist)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, "the call allocates"
    torch.cuda.current_stream().wait_stream(side)
    _sync("warmed sln_mesh_retrieve")
    want, want_d = choice.clone(), dist.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        RT.into(b, o, rr, table, choice, dist)
    for _ in range(2):
        choice.fill_(-5); dist.zero_()
        graph.replay()
        _sync("replay of sln_mesh_retrieve")
        assert torch.equal(choice, want) and _same_bits(torch.nan_to_num(dist, nan=-1.0), torch.nan_to_num(want_d, nan=-1.0))
    assert torch.equal(want.cpu(), RT.retrieve_models_torch(torch.from_numpy(boxes), torch.from_numpy(objs), torch.from_numpy(room_row),
                                                           RT.ModelTable(data, vocab)))
