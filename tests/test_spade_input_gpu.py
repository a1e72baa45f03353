"""The device input builder (csrc/spade_input.hip through host/spade_input.py::InputBuilder, run with -m gpu) against the tensor the
reference's own ``colorize_with_spade`` produced (tests/golden/spade_input.npz), against the ATen restatement ``build_input`` on the
same device tensors, and - where the resize is the identity - bit for bit against the numpy lines of the oracle."""
import numpy as np
import pytest
import torch

from conftest import load_golden, pkg
from oracle import spade_input_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-6                                  # the bound tests/test_spade_input.py holds build_input to


def _device_scene(depth, masks, dtype=torch.uint8):
    names = list(masks)
    planes = torch.from_numpy(np.stack([masks[k] for k in names])).to(dtype).cuda()
    return torch.from_numpy(depth).cuda(), planes, names


def _assert_close(got, want, what):
    got, want = got.double().cpu().numpy(), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("%s: largest error / max(1, |want|) = %.3e" % (what, err.max()))
    assert err.max() <= TOL, (what, err.max())


def test_golden_fixture_of_the_reference_function():
    S = pkg("host.spade_input")
    g = load_golden("spade_input")
    depth, masks = R.synth_scene(1024, seed=2)
    want_half, chans = g["total_half"], g["total_channels"]
    d, planes, names = _device_scene(depth, masks)
    assert np.array_equal(planes.float().cpu().numpy(), np.stack([masks[k] for k in names]))        # the scene's masks are whole bytes
    got = S.InputBuilder(1024, 1024, size=256)(d, masks=planes, channels=names)
    assert got.shape == (1, 41, 256, 256) and got.dtype == torch.float32
    _assert_close(got[0][torch.from_numpy(chans).cuda()][:, ::2, ::2], want_half, "live channels at [::2, ::2]")
    sums = got[0].double().reshape(41, -1).sum(1).cpu().numpy()
    print("largest per-channel sum error %.3e" % np.abs(sums - g["total_sums"]).max())
    assert np.abs(sums - g["total_sums"]).max() <= TOL * 256 * 256
    assert sorted(chans.tolist()) == sorted([0] + [1 + S.NYU40.index(k) for k in names])


def _scene_hw(H, W, seed=0):
    depth, masks = R.synth_scene(max(H, W), seed=seed)
    return np.ascontiguousarray(depth[:H, :W]), {k: np.ascontiguousarray(v[:H, :W]) for k, v in masks.items()}


@pytest.mark.parametrize("H,W,size", [(1024, 1024, 256), (512, 512, 256), (768, 768, 256), (1000, 1000, 256), (256, 256, 256), (768, 1024, 256),
                                      (256, 256, 64)])
def test_against_build_input_on_the_same_tensors(H, W, size):
    S = pkg("host.spade_input")
    depth, masks = _scene_hw(H, W, seed=H + W)
    d, planes, names = _device_scene(depth, masks)
    want = S.build_input(d, {k: planes[j] for j, k in enumerate(names)}, size=size)
    got = S.InputBuilder(H, W, size=size)(d, masks=planes, channels=names)
    assert got.shape == want.shape == (1, 41, size, size)
    _assert_close(got, want.cpu().numpy(), "%d x %d -> %d" % (H, W, size))
    got32 = S.InputBuilder(H, W, size=size)(d, masks=planes.float(), channels=names)
    assert torch.equal(got32, got)


def test_values_before_the_resize_are_the_oracles_bit_for_bit():
    """H = W = size: the resize is the identity, what is left is the float32 operation order of the normalisation
    (oracle/spade_input_ref.py:42-46) and the 120 rule (:50-52)"""
    S = pkg("host.spade_input")
    depth, masks = R.synth_scene(256, seed=5)
    d = depth - np.min(depth)
    dmax = np.max(d[d < 20])
    d = np.clip(d, 0, dmax) / dmax
    want = np.zeros((41, 256, 256), np.float32)
    want[0] = ((d - 0.5) * 2).astype("float32")
    for name, m in masks.items():
        buf = m.astype("float32").copy()
        buf[buf < 120] = 0.0
        buf[buf > 120] = 1.0
        want[1 + R.NYU40.index(name)] = buf
    dd, planes, names = _device_scene(depth, masks)
    got = S.InputBuilder(256, 256, size=256)(dd, masks=planes, channels=names)[0].cpu().numpy()
    assert (want == 120).any() and (got == 120).sum() == (want == 120).sum()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()


def _one_hot_scene(n, seed, classes=(0, 1, 4, 32, 40)):
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.repeat(rng.choice(np.array(classes, np.uint8), size=(n // 8, n // 8)), 8, 0), 8, 1)
    depth = (1.0 + 4.0 * rng.random((n, n))).astype(np.float32)
    return torch.from_numpy(depth).cuda(), torch.from_numpy(labels).cuda()


def test_uint8_float32_and_label_forms_agree_bit_for_bit():
    S = pkg("host.spade_input")
    d, labels = _one_hot_scene(256, 1)
    masks = S.masks_from_labels(labels)
    names = list(masks)
    planes = torch.stack([masks[k] for k in names])
    b = S.InputBuilder(256, 256, size=64)
    from_u8 = b(d, masks=planes, channels=names).clone()
    from_f32 = b(d, masks=planes.float(), channels=names).clone()
    from_labels = b(d, labels=labels).clone()
    assert from_u8[0, 1 + S.NYU40.index("bed")].max() > 0.5
    assert torch.equal(from_u8, from_f32) and torch.equal(from_u8, from_labels)
    want = S.build_input(d, {k: planes[j] for j, k in enumerate(names)}, size=64)
    _assert_close(from_labels, want.cpu().numpy(), "label form")


def test_absent_channels_are_written_as_zero():
    S = pkg("host.spade_input")
    depth, masks = R.synth_scene(256, seed=3)
    d, planes, names = _device_scene(depth, masks)
    b = S.InputBuilder(256, 256, size=64)
    live = [0] + [1 + S.NYU40.index(k) for k in names]
    absent = [c for c in range(41) if c not in live]
    for kwargs in (dict(masks=planes, channels=names), dict(labels=S.labels_from_masks({k: planes[j] for j, k in enumerate(names) if k != "wall"})),
                   dict()):
        b.out.fill_(float("nan"))
        got = b(d, **kwargs)
        assert not torch.isnan(got).any()
        dead = absent if kwargs else list(range(1, 41))
        assert (got[0, dead] == 0).all() and not torch.signbit(got[0, dead]).any()
    assert got[0, 0].abs().max() > 0.5


def test_batch_of_three_equals_three_single_calls_and_repeats():
    S = pkg("host.spade_input")
    rooms = []
    for seed, keep, scale in ((1, ("bed", "wall"), 1.0), (2, ("night_stand",), 0.25), (3, ("bed", "night_stand", "wall", "floor_mat"), 3.0)):
        depth, masks = R.synth_scene(256, seed=seed)
        depth = depth * scale
        depth[:8, :8] = 65504.0
        rooms.append((depth, {k: masks[k] for k in keep}))
    n = 4
    planes = torch.zeros(3, n, 256, 256, dtype=torch.uint8).cuda()
    planes[1, 1:] = 77                                                          # padding planes are not read
    names = []
    for r, (_, m) in enumerate(rooms):
        for j, k in enumerate(m):
            planes[r, j] = torch.from_numpy(m[k]).to(torch.uint8)
        names.append(list(m) + [None] * (n - len(m)))
    depths = torch.from_numpy(np.stack([r[0] for r in rooms])).cuda()
    b3 = S.InputBuilder(256, 256, size=64, batch=3)
    first = b3(depths, masks=planes, channels=names).clone()
    second = b3(depths, masks=planes, channels=names)
    assert torch.equal(first, second)
    b1 = S.InputBuilder(256, 256, size=64)
    for r, (depth, m) in enumerate(rooms):
        d, pl, nm = _device_scene(depth, m)
        one = b1(d, masks=pl, channels=nm)
        assert torch.equal(one[0], first[r]), r
        _assert_close(one, S.build_input(d, {k: pl[j] for j, k in enumerate(nm)}, size=64).cpu().numpy(), "room %d" % r)
    assert b3.status.tolist() == [0, 0, 0]
    listed = S.build_inputs([torch.from_numpy(r[0]).cuda() for r in rooms], [{k: torch.from_numpy(v).to(torch.uint8).cuda() for k, v in r[1].items()}
                                                                              for r in rooms], size=64)
    assert torch.equal(listed, first)


def test_side_stream_and_linear_graph_capture():
    S = pkg("host.spade_input")
    sceneA, sceneB = R.synth_scene(256, seed=7), R.synth_scene(256, seed=8)
    dA, pA, names = _device_scene(*sceneA)
    dB, pB, _ = _device_scene(sceneB[0] * 1.5, sceneB[1])
    chan = torch.tensor([[S.NYU40.index(k) for k in names]], dtype=torch.int32).cuda()
    ref = S.InputBuilder(256, 256, size=64)
    wantA, wantB = ref(dA, masks=pA, channels=names).clone(), ref(dB, masks=pB, channels=names).clone()
    assert not torch.equal(wantA, wantB)
    b = S.InputBuilder(256, 256, size=64)
    d, p = dA.clone(), pA.clone()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        assert torch.equal(b(d, masks=p, channels=chan), wantA)                 # eager, on a stream that is not the default one
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    b.out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b(d, masks=p, channels=chan)
    graph.replay()
    assert torch.equal(b.out, wantA)
    d.copy_(dB); p.copy_(pB)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(b.out, wantB)


def test_no_depth_below_twenty_sets_the_status_word():
    """The selection d[d < 20] is empty only when no d - min compares below 20 - the minimum itself gives 0, so that needs a depth map
    without a finite value (a render whose every ray left the scene: inf).  The reference raises there."""
    S = pkg("host.spade_input")
    depth, masks = R.synth_scene(64, seed=1)
    nothing = np.full_like(depth, np.inf)
    with pytest.raises(ValueError):
        with np.errstate(invalid="ignore"):
            R.build_input(nothing, masks, size=32)
    d, planes, names = _device_scene(nothing, masks)
    good = torch.from_numpy(depth).cuda()
    quiet = S.InputBuilder(64, 64, size=32)
    got = quiet(d, masks=planes, channels=names)                                # the default neither raises nor reads the word
    assert quiet.status.tolist() == [1]
    assert torch.isnan(got[0, 0]).all() and not torch.isnan(got[0, 1:]).any()
    quiet(good, masks=planes, channels=names)
    assert quiet.status.tolist() == [0] and not torch.isnan(quiet.out).any()
    strict = S.InputBuilder(64, 64, size=32, validate=True)
    strict(good, masks=planes, channels=names)
    with pytest.raises(ValueError):
        strict(d, masks=planes, channels=names)
    two = S.InputBuilder(64, 64, size=32, batch=2)
    two(torch.stack([good, d]), labels=torch.zeros(2, 64, 64, dtype=torch.uint8).cuda())
    assert two.status.tolist() == [0, 1]


def test_colorize_rooms_is_the_builder_and_one_colorize_call_per_room():
    from oracle import spade_ref
    from oracle.gen_golden_spade import CASES
    S = pkg("host.spade_input"); G4 = pkg("host.SPADE_related")
    cfg = spade_ref.SpadeConfig(**CASES["spade_small"][0])
    G = G4.SPADEGenerator4(cfg.semantic_nc, cfg.target_nc, cfg.nz, cfg.ngf, 'spectralspadelayer3x3', cfg.crop_size, 'normal')
    G.load_state_dict(spade_ref.init_state(cfg, seed=7)); G = G.cuda().eval()
    n = 4 * cfg.crop_size
    builder = S.InputBuilder(n, n, size=cfg.crop_size)
    rooms = []
    for seed in (1, 2):
        depth, masks = _scene_hw(n, n, seed=seed)
        d, planes, names = _device_scene(depth, masks)
        rooms.append(dict(depth=d, masks=planes, channels=names))
    d, labels = _one_hot_scene(n, 3)
    rooms[1] = dict(depth=d, labels=labels)                                     # the second room arrives as a class-index image
    imgs = S.colorize_rooms(G, builder, rooms, 3, generator=torch.Generator(device="cuda").manual_seed(0))
    assert imgs.shape == (2, 3, cfg.crop_size, cfg.crop_size, 3) and imgs.dtype == torch.uint8 and imgs.is_cuda
    gen = torch.Generator(device="cuda").manual_seed(0)
    for r, room in enumerate(rooms):
        assert torch.equal(imgs[r], S.to_uint8(S.colorize(G, builder(**room), 3, gen))), r
    assert not torch.equal(imgs[0], imgs[1])
