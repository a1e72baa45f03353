"""State-keeping of the library around its kernels (round-5 advisor findings): W^T validity of a room group, the engines' buffers
after a group is gone, the split scratch of small SPADE convolutions (slots, release, capture), the side-stream picks, and the
geometry check of the per-room loss."""
import ctypes as C
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import pkg
from parity import assert_close

pytestmark = pytest.mark.gpu

from oracle import vae_ref     # noqa: E402   (state / batch generators only)


def _rooms(n_rooms, dev="cuda"):
    syn = pkg("host.synthetic")
    names = ["bed", "chair", "table", "sofa", "desk", "__room__"]
    rooms = []
    for r in range(n_rooms):
        g = torch.Generator().manual_seed(100 + r)
        n = len(names)
        lo = torch.rand(n, 3, generator=g) * 0.45 + 0.05
        lo[:, 1] = 0.0
        boxes = torch.cat([lo, lo + torch.rand(n, 3, generator=g) * 0.2 + 0.12], 1)
        boxes[-1] = torch.tensor([0, 0, 0, 4.0, 2.7, 5.0])
        tri = torch.tensor([[0, 1, 1], [2, 3, 3]] + [[i, 0, n - 1] for i in range(n - 1)])
        rooms.append(dict(objs=torch.tensor([3, 4, 6, 5, 7, 0]).to(dev), triples=tri.to(dev), boxes=boxes.to(dev),
                          angles=torch.randint(0, 24, (n,), generator=g).to(dev), attributes=torch.zeros(n, dtype=torch.int64, device=dev),
                          class_names=names))
    return rooms


def _model():
    M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2)
    m = M.Sg2ScVAEModel(**cfg.model_kwargs())
    m.load_state_dict(vae_ref.init_state(cfg, seed=1))
    return m.cuda().eval()


# Upstream gradients of the decoder's outputs, scaled so that one fused SGD step (1.1e-5 x the wgrad) moves W far enough that a
# backward with the W^T of the previous weights gives a dz that is off by much more than the comparisons' tolerance (measured in
# the tests: `moved`)
_UPSTREAM = 1e3


def _upstream(rb):
    gen = torch.Generator(device="cuda").manual_seed(11)
    rb.d_boxes_pred.normal_(generator=gen).mul_(_UPSTREAM); rb.d_angles_pred.normal_(generator=gen).mul_(_UPSTREAM)


class _MixLinear(torch.autograd.Function):
    """y = x W_act^T + b forward, dx = dy W_bwd backward: a backward that finds no forward in front of it runs its dgrads with the
    W^T of the CURRENT weights against the activations the last forward saved (at the weights of that time)"""
    @staticmethod
    def forward(ctx, x, w, b, w_bwd):
        ctx.save_for_backward(x, w_bwd)
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w_bwd = ctx.saved_tensors
        return dy @ w_bwd, dy.t() @ x, dy.sum(0), None


def _room_params(model, flat):
    """name -> fp64 CPU tensor of one room's flat parameter row (the model's named_parameters() offsets into flat_params)"""
    base = model.flat_params.data_ptr()
    out = {}
    for name, t in model.named_parameters():
        off = (t.data_ptr() - base) // 4
        out[name] = flat[off:off + t.numel()].reshape(t.shape).detach().double().cpu()
    return out


def _decoder_oracle(model, rb, rooms, r, p_act, p_bwd):
    """fp64 decoder of room r (oracle/vae_ref.decoder, eval mode) at the parameter row p_act, backward from the group's upstream
    gradients with every Linear's dgrad taken at p_bwd -> (dz [n, E], {parameter name: gradient})"""
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2)
    sd = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}
    act, bwd = _room_params(model, p_act), _room_params(model, p_bwd)
    leaves = {}
    for name, v in act.items():
        sd[name] = leaves[name] = v.clone().requires_grad_(True)
    w_bwd = {id(sd[n]): bwd[n] for n in act if n.endswith(".weight")}

    class Fshim:
        def __getattr__(self, a):
            return getattr(F, a)

        @staticmethod
        def linear(x, w, b=None):
            return _MixLinear.apply(x, w, b, w_bwd[id(w)])
    a, n = rb.row0[r], rb.rows[r]
    z = rb.z[a:a + n].detach().double().cpu().requires_grad_(True)
    rm = rooms[r]
    with mock.patch.object(vae_ref, "F", Fshim()):
        boxes, angles = vae_ref.decoder(sd, cfg, z, rm["objs"].cpu(), rm["triples"].cpu(), rm["attributes"].cpu(), False)
    db = rb.d_boxes_pred[a:a + n, :boxes.shape[1]].double().cpu()
    da = rb.d_angles_pred[a:a + n].double().cpu()            # the gradient of the LOG-SOFTMAX output (the group differentiates it)
    torch.autograd.backward([boxes, angles], [db, da])
    return z.grad, {k: v.grad for k, v in leaves.items() if v.grad is not None}


def _fused_names(model, rb):
    """names of the parameter tensors the group's wgrad launches step themselves (sln_vae_group_fused_params, room 0's pointers)"""
    lib = pkg("_lib").lib()
    nf = int(lib.sln_vae_group_fused_params(rb._group, None, None, 0))
    ptrs, lens = (C.c_void_p * nf)(), (C.c_int64 * nf)()
    lib.sln_vae_group_fused_params(rb._group, ptrs, lens, nf)
    by_off = {(t.data_ptr() - model.flat_params.data_ptr()) // 4: name for name, t in model.named_parameters()}
    base = rb.params.data_ptr()
    return [by_off[(int(ptrs[i]) - base) // 4] for i in range(nf)]


@pytest.mark.parametrize("R", [2, 5])
def test_group_backward_rebuilds_w_transposed_when_no_forward_left_a_valid_one(R):
    """forward builds W^T (side stream from 4 rooms on); the backward's fused wgrads step W, so a second backward - or one without a
    forward in front - must transpose again.  Counted with sln_vae_group_transposes; the second backward's dz and parameter step must
    equal the fp64 decoder (oracle/vae_ref) evaluated as that backward mixes it: activations of the first forward (the parameters of
    construction), dgrads with the W^T of the parameters the first backward left."""
    Rf = pkg("host.refine"); L = pkg("_lib")
    lib = L.lib()
    model = _model()
    rooms = _rooms(R)
    rb = Rf.RefineBatch(model, rooms, image_size=96, iters=3)
    try:
        st = L.current_stream_ptr()
        g = rb._group
        params0 = rb.params.clone()
        n0 = lib.sln_vae_group_transposes(g)
        L.check(lib.sln_vae_group_decoder(g, st), "fwd"); torch.cuda.synchronize()
        assert lib.sln_vae_group_transposes(g) == n0 + 1
        _upstream(rb)
        L.check(lib.sln_vae_group_decoder_backward(g, st), "bwd"); torch.cuda.synchronize()
        assert lib.sln_vae_group_transposes(g) == n0 + 1, "a backward behind a forward uses the forward's W^T"
        params_after_first = rb.params.clone()
        L.check(lib.sln_vae_group_decoder_backward(g, st), "bwd 2"); torch.cuda.synchronize()
        assert lib.sln_vae_group_transposes(g) == n0 + 2, "the second backward found W^T stale (the first one stepped W) and rebuilt it"
        dz2 = rb.dz.clone()
        assert torch.isfinite(dz2).all() and float(dz2.abs().max()) > 0
        assert not torch.equal(params_after_first, rb.params), "the fused wgrads stepped the parameters again"
        step = float(rb._step)
        fused = _fused_names(model, rb)
        assert fused
        base = model.flat_params.data_ptr()
        for r in range(R):
            a, n = rb.row0[r], rb.rows[r]
            dz_ref, grads = _decoder_oracle(model, rb, rooms, r, params0[r], params_after_first[r])
            assert_close(dz2[a:a + n].cpu().numpy(), dz_ref.numpy(), "room %d: dz of the second backward" % r, rtol=1e-4)
            # a stale W^T (the first forward's) would give the FIRST backward's dz again: far outside that bound
            dz_stale, _ = _decoder_oracle(model, rb, rooms, r, params0[r], params0[r])
            moved = float((dz_stale - dz_ref).abs().max()) / float(dz_ref.abs().max())
            assert moved > 10 * 1e-4, "a stale W^T moves dz by %.2e only: the comparison above would not see it" % moved
            for name in fused:
                t = dict(model.named_parameters())[name]
                off = (t.data_ptr() - base) // 4
                mid = params_after_first[r, off:off + t.numel()].double().cpu()
                got = rb.params[r, off:off + t.numel()].double().cpu() - mid
                want = -step * grads[name].reshape(-1)
                ulp = float(np.spacing(np.float32(mid.abs().max())))        # the step lands in an fp32 parameter: rounded to its ulp
                assert_close(got.numpy(), want.numpy(), "room %d: step of %s" % (r, name), rtol=1e-4, atol=ulp)
    finally:
        rb.close()


def _det_batch(R):
    L = pkg("_lib")
    L.check(L.lib().sln_set_deterministic(1), "sln_set_deterministic")
    rb = pkg("host.refine").RefineBatch(_model(), _rooms(R), image_size=96, iters=3)
    _upstream(rb)
    return rb


def _state(rb):
    torch.cuda.synchronize()
    return rb.dz.clone(), rb.params.clone(), rb.boxes_pred.clone()


def _eager_fwd_bwd_bwd(R):
    """the eager sequence forward, backward, backward (its second backward is pinned to the fp64 oracle by the test above) ->
    (state after the first backward, state after the second)"""
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    rb = _det_batch(R)
    try:
        L.check(lib.sln_vae_group_decoder(rb._group, st), "fwd")
        L.check(lib.sln_vae_group_decoder_backward(rb._group, st), "bwd")
        one = _state(rb)
        L.check(lib.sln_vae_group_decoder_backward(rb._group, st), "bwd 2")
        return one, _state(rb)
    finally:
        lib.sln_set_deterministic(0)
        rb.close()


def _assert_same_state(got, want, first, what):
    for name, a, b in zip(("dz", "params", "boxes_pred"), got, want):
        assert torch.equal(a, b), "%s: %s differs from the eager forward, backward, backward (max %.3e)" % (what, name, float((a - b).abs().max()))
    # what a stale W^T costs: the second backward's dz would be the first one's again, which differs from it by far more than the
    # bit-exactness asked above (see _UPSTREAM)
    moved = float((first[0] - want[0]).abs().max()) / float(want[0].abs().max())
    assert moved > 1e-3, moved


def _capture(fn, stream):
    L = pkg("_lib")
    assert L.lib().sln_side_stream_prepare(C.c_void_p(stream.cuda_stream)) in (0, 1)
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        L.check(fn(C.c_void_p(stream.cuda_stream)), "captured call")
    return g


# (R = 2: the group keeps its side stream off below four rooms, so eager and captured calls take the same one-stream order)
@pytest.mark.parametrize("R", [2])
def test_captured_forward_does_not_validate_w_transposed_for_an_eager_backward(R):
    """a forward that is only RECORDED (captured, never replayed) built no W^T: the eager backward behind it must transpose"""
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    first, want = _eager_fwd_bwd_bwd(R)
    rb = _det_batch(R)
    try:
        g = rb._group
        L.check(lib.sln_vae_group_decoder(g, st), "fwd")
        L.check(lib.sln_vae_group_decoder_backward(g, st), "bwd")
        graph = _capture(lambda s: lib.sln_vae_group_decoder(g, s), torch.cuda.Stream())
        torch.cuda.synchronize()
        n = lib.sln_vae_group_transposes(g)
        L.check(lib.sln_vae_group_decoder_backward(g, st), "eager bwd behind a captured fwd")
        assert lib.sln_vae_group_transposes(g) == n + 1, "the eager backward rebuilt W^T"
        _assert_same_state(_state(rb), want, first, "captured fwd, eager bwd")
        del graph
    finally:
        L.lib().sln_set_deterministic(0)
        rb.close()


@pytest.mark.parametrize("R", [2])
def test_backward_only_graph_replayed_twice_transposes_in_every_replay(R):
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    first, want = _eager_fwd_bwd_bwd(R)
    rb = _det_batch(R)
    try:
        g = rb._group
        L.check(lib.sln_vae_group_decoder(g, st), "fwd")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        graph = _capture(lambda p: lib.sln_vae_group_decoder_backward(g, p), s)
        graph.replay(); graph.replay()
        _assert_same_state(_state(rb), want, first, "backward graph replayed twice")
        del graph
    finally:
        L.lib().sln_set_deterministic(0)
        rb.close()


@pytest.mark.parametrize("R", [2])
def test_eager_backward_after_a_replayed_backward_graph_transposes(R):
    """a replay steps W behind the host's back: an eager backward behind it - even with an eager forward in between capture and
    replay - must not trust the forward's W^T"""
    L = pkg("_lib")
    lib, st = L.lib(), L.current_stream_ptr()
    first, want = _eager_fwd_bwd_bwd(R)
    rb = _det_batch(R)
    try:
        g = rb._group
        s = torch.cuda.Stream()
        graph = _capture(lambda p: lib.sln_vae_group_decoder_backward(g, p), s)
        L.check(lib.sln_vae_group_decoder(g, st), "fwd")
        graph.replay()
        L.check(lib.sln_vae_group_decoder_backward(g, st), "eager bwd behind a replayed bwd")
        _assert_same_state(_state(rb), want, first, "replayed bwd graph, eager bwd")
        del graph
    finally:
        L.lib().sln_set_deterministic(0)
        rb.close()


def test_refine_graph_keeps_one_transposition():
    """RefineBatch.run(capture=True) records forward and backward in ONE capture: the backward reuses that capture's W^T"""
    Rf = pkg("host.refine"); L = pkg("_lib")
    lib = L.lib()
    rb = Rf.RefineBatch(_model(), _rooms(2), image_size=96, iters=4)
    try:
        g = rb._group
        rb.run(1, capture=True)                 # first iterate's sizes (one forward) + eager warm-up iteration (forward, backward) + capture
        torch.cuda.synchronize()
        assert lib.sln_vae_group_transposes(g) == 3, "sizes pass 1, warm-up forward 1, captured forward 1, captured backward 0"
        rb.run(2, capture=True)
        torch.cuda.synchronize()
        assert lib.sln_vae_group_transposes(g) == 3, "replays do not pass through the host"
    finally:
        rb.close()


def test_engines_get_their_own_buffers_back_when_the_group_goes():
    """sln_vae_group_create redirects the engines' decoder outputs into group-owned arrays; destroy puts the engines' own back: a
    decoder call on a bare engine afterwards must not touch freed memory (it writes its own workspace again)."""
    Rf = pkg("host.refine"); L = pkg("_lib")
    lib = L.lib()
    model = _model()
    rooms = _rooms(2)
    rb = Rf.RefineBatch(model, rooms, image_size=96, iters=2)
    rb.run(1)
    torch.cuda.synchronize()
    engines = list(rb._engines)
    lib.sln_vae_group_destroy(rb._group); rb._group = None
    # the group's arrays may be reused by the allocator now
    del rb.boxes_pred, rb.angles_pred
    junk = [torch.full((1 << 16,), float("nan"), device="cuda") for _ in range(8)]
    z = torch.randn(6, 32, device="cuda")
    out_b, out_a = torch.empty(6, 6, device="cuda"), torch.empty(6, 24, device="cuda")
    h = engines[0][0]
    r = lib.sln_vae_decoder(h, L.ptr(z), L.ptr(out_b), L.ptr(out_a), 0, L.current_stream_ptr())
    torch.cuda.synchronize()
    assert r == 0 and torch.isfinite(out_b).all() and torch.isfinite(out_a).all()
    assert all(torch.isnan(j).all() for j in junk), "an engine wrote into memory the group had owned"
    for e in engines:
        lib.sln_vae_destroy(e[0])
    rb._engines = []


def test_split_scratch_slots_release_lru_and_capture_error():
    L = pkg("_lib"); S = pkg("host.SPADE_related")
    lib = L.lib()
    Cin, Cout, H = 1024, 256, 8
    g = torch.Generator().manual_seed(7)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    wp, rp = S._pack(w.cuda())
    bp = torch.zeros(rp, device="cuda")
    x = torch.randn(1, Cin, H, H, generator=g).cuda()

    def conv(y, st):
        return lib.sln_spade_conv(L.ptr(x), 1, Cin, H, H, L.ptr(wp), L.ptr(bp), Cout, rp, 3, 0, 0.0, L.ptr(y), C.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    lib.sln_spade_release(None, 1)
    free0 = torch.cuda.mem_get_info()[0]
    streams = [torch.cuda.Stream() for _ in range(20)]          # more streams than slots (16): the least recently used slots are recycled
    ys = []
    for st in streams:
        y = torch.empty(1, Cout, H, H, device="cuda")
        assert conv(y, st) == 0
        ys.append(y)
    torch.cuda.synchronize()
    assert all(torch.equal(y, ys[0]) for y in ys), "a split launch gives the same bits on every stream, recycled slot or not"
    held = free0 - torch.cuda.mem_get_info()[0]
    assert held <= 17 * (48 << 20), "at most 16 slots of 48 MB are alive (%d MB held)" % (held >> 20)
    assert lib.sln_spade_release(C.c_void_p(streams[-1].cuda_stream), 0) == 1
    assert lib.sln_spade_release(C.c_void_p(streams[-1].cuda_stream), 0) == 0
    n = lib.sln_spade_release(None, 1)
    assert n == 15
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < (48 << 20), "release gives the memory back"
    # a stream first seen while it is captured: the split launch FAILS (it used to run another kernel with other rounding, silently)
    fresh = torch.cuda.Stream()
    y = torch.empty(1, Cout, H, H, device="cuda")
    graph = torch.cuda.CUDAGraph()
    fresh.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=fresh):
        rc = conv(y, fresh)
    assert rc == -3, rc
    # prepared first, the same capture records the split launch and replays to the eager bits
    assert lib.sln_spade_prepare(C.c_void_p(fresh.cuda_stream)) == 0
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=fresh):
        rc = conv(y, fresh)
    assert rc == 0
    y.zero_(); graph2.replay(); torch.cuda.synchronize()
    assert torch.equal(y, ys[0])
    # graph2 recorded a split launch on `fresh`: that slot is pinned - a plain release leaves it, the explicit one frees it once the
    # graph is gone
    assert lib.sln_spade_release(C.c_void_p(fresh.cuda_stream), 0) == 0
    assert lib.sln_spade_release(None, 1) == 0
    del graph2
    assert lib.sln_spade_release(C.c_void_p(fresh.cuda_stream), 2) == 1       # SLN_SPADE_RELEASE_PINNED
    assert lib.sln_spade_release(None, 3) == 0


def _split_conv_case():
    """a convolution small enough to take the input-channel split (the shape of the test above) -> (x, w, conv(y, stream))"""
    L = pkg("_lib"); S = pkg("host.SPADE_related")
    lib = L.lib()
    Cin, Cout, H = 1024, 256, 8
    g = torch.Generator().manual_seed(7)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    wp, rp = S._pack(w.cuda())
    bp = torch.zeros(rp, device="cuda")
    x = torch.randn(1, Cin, H, H, generator=g).cuda()

    def conv(y, st):
        return lib.sln_spade_conv(L.ptr(x), 1, Cin, H, H, L.ptr(wp), L.ptr(bp), Cout, rp, 3, 0, 0.0, L.ptr(y), C.c_void_p(st.cuda_stream))
    return x, w, conv


def _evict_split_slots(n=20):
    """split launches on n fresh streams (more than the 16 slots: the least recently used unpinned slots are recycled), then a
    plain release of every slot"""
    _, _, conv = _split_conv_case()
    streams = [torch.cuda.Stream() for _ in range(n)]
    for st in streams:
        assert conv(torch.empty(1, 256, 8, 8, device="cuda"), st) == 0
    torch.cuda.synchronize()
    pkg("_lib").lib().sln_spade_release(None, 1)


def _slot_alive(stream):
    """does `stream` own a split-scratch slot?  sln_spade_prepare on a stream that is being captured finds an existing slot (0) and
    cannot allocate one (SLN_E_STATE): a look-up that allocates nothing and launches nothing of the library"""
    lib = pkg("_lib").lib()
    g = torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=stream):
        rc = lib.sln_spade_prepare(C.c_void_p(stream.cuda_stream))
        torch.zeros(1, device="cuda").add_(1)
    assert rc in (0, -3), rc
    return rc == 0


def test_a_captured_split_launch_keeps_its_scratch_slot_through_eviction_and_release():
    """the graph holds the address of its stream's slot: 20 other streams' split launches (LRU eviction) and a release of every slot
    must leave that slot alive.  Liveness is asserted BEFORE the replay: a graph is never replayed into freed memory."""
    lib = pkg("_lib").lib()
    x, w, conv = _split_conv_case()
    lib.sln_spade_release(None, 1)
    eager = torch.empty(1, 256, 8, 8, device="cuda")
    assert conv(eager, torch.cuda.current_stream()) == 0
    s = torch.cuda.Stream()
    assert lib.sln_spade_prepare(C.c_void_p(s.cuda_stream)) == 0
    y = torch.zeros(1, 256, 8, 8, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, stream=s):
            rc = conv(y, s)
        assert rc == 0
        _evict_split_slots()
        assert _slot_alive(s), "the captured stream's split scratch was freed while its graph holds it"
        y.zero_(); graph.replay(); torch.cuda.synchronize()
        assert torch.equal(y, eager), "the replay gives the eager bits"
        ref = F.conv2d(F.pad(x.double().cpu(), (1, 1, 1, 1), mode="reflect"), w.double())
        assert_close(y.cpu().numpy(), ref.numpy(), "replayed split conv vs fp64", rtol=1e-4)
    finally:
        del graph
        torch.cuda.synchronize()
        lib.sln_spade_release(C.c_void_p(s.cuda_stream), 2)
        lib.sln_spade_release(None, 1)


def test_generator_graph_keeps_its_split_scratch_slot_through_eviction_and_release():
    """SPADEGenerator4's captured batch-1 call (graph_batch1) on its own stream: the same liveness before a replay, the replay's bits
    unchanged and within 1e-4 of the fp64 oracle; clear_map_cache() drops the graph and frees the slot"""
    from oracle import spade_ref
    from oracle.gen_golden_spade import CASES
    S = pkg("host.SPADE_related")
    lib = pkg("_lib").lib()
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    sd = spade_ref.init_state(cfg, seed=7)
    G = S.SPADEGenerator4(cfg.semantic_nc, cfg.target_nc, cfg.nz, cfg.ngf, 'spectralspadelayer3x3', cfg.crop_size, 'normal')
    G.load_state_dict(sd); G = G.cuda().eval()
    G.graph_batch1 = True
    seg, _ = spade_ref.synth_input(cfg, 1, seed=5)
    zs = torch.from_numpy(np.random.default_rng(4).standard_normal((2, cfg.nz)).astype(np.float32))
    ref = spade_ref.generator(sd, cfg, seg, zs).numpy()
    total = seg.cuda()
    lib.sln_spade_release(None, 1)
    try:
        for _ in range(3):                                   # calls 1, 2 eager on the module's stream, call 3 captured
            G(total, zs[:1].cuda())
        assert G._b1_graph is not None and G._b1_graph["graph"] is not None
        s = G._b1_stream
        want = G(total, zs[1:2].cuda())
        torch.cuda.synchronize()
        _evict_split_slots()
        assert _slot_alive(s), "the generator's capture stream lost its split scratch while its graph holds it"
        got = G(total, zs[1:2].cuda())
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        assert_close(got.cpu().numpy(), ref[1:2], "replayed generator call vs fp64", rtol=1e-4, atol=1e-4)
        G.clear_map_cache()
        assert not _slot_alive(s), "clear_map_cache() dropped the graph and freed its slot"
    finally:
        G.clear_map_cache()
        lib.sln_spade_release(None, 1)


def test_side_stream_pick_survives_streams_that_come_and_go():
    """the pick of a caller stream is probed, aged and can be forgotten: after eight streams were created and destroyed (their handles
    may come back on other hardware queues) a new caller stream still gets a side stream that a probe sees overlapping"""
    L = pkg("_lib")
    lib = L.lib()
    idx, ov = C.c_int(-1), C.c_int(-1)
    cur = torch.cuda.Stream()
    with torch.cuda.stream(cur):
        assert lib.sln_side_stream_prepare(C.c_void_p(cur.cuda_stream)) in (0, 1)
        rc = lib.sln_debug_side_stream(C.c_void_p(cur.cuda_stream), C.byref(idx), C.byref(ov))
    had = rc == 0 and ov.value == 1
    for _ in range(8):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            lib.sln_side_stream_prepare(C.c_void_p(s.cuda_stream))
            torch.zeros(8, device="cuda").add_(1)
        s.synchronize()
        assert lib.sln_side_stream_forget(C.c_void_p(s.cuda_stream)) == 1
        assert lib.sln_side_stream_forget(C.c_void_p(s.cuda_stream)) == 0
        del s
    nxt = torch.cuda.Stream()
    with torch.cuda.stream(nxt):
        got = lib.sln_side_stream_prepare(C.c_void_p(nxt.cuda_stream))
        rc = lib.sln_debug_side_stream(C.c_void_p(nxt.cuda_stream), C.byref(idx), C.byref(ov))
    if had:                       # (a box with one hardware queue has no overlap to keep: nothing to assert there)
        assert got == 1 and rc == 0 and ov.value == 1
    # a prepare inside a capture is refused, not performed
    g = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    cap.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=cap):
        rc = lib.sln_side_stream_prepare(C.c_void_p(cap.cuda_stream))
        torch.zeros(8, device="cuda").add_(1)
    assert rc == -3


def test_per_room_loss_refuses_an_unsupported_geometry_before_any_launch():
    R = pkg("host.refine"); L = pkg("_lib")
    tgt = torch.zeros(2, 70, 64, 64, device="cuda")
    with pytest.raises(L.SlnError):
        R.RefineLoss(tgt, sizes=(30,), per_room=True)           # 1 x 30 x 30 rows per room: not a multiple of the loss kernel's 128-row blocks
    R.RefineLoss(tgt, sizes=(30,), per_room=False)
    R.RefineLoss(tgt, sizes=(32, 48), per_room=True)
