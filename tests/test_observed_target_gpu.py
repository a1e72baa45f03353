"""csrc/observed_target.hip on the device against host/observe.py::observed_target_torch (every operation of the definition is exact or
correctly rounded: equal bits are asked for), its repeatability, its refusals, and a round trip against the device scene pass."""
import ctypes as C

import numpy as np
import pytest
import torch

import observed_cases as OC
from conftest import pkg
from oracle import vae_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = OC.cases()
_YARDSTICK = {}


def _yardstick(case):
    """the torch definition on the CPU, once per case"""
    if case["name"] not in _YARDSTICK:
        _YARDSTICK[case["name"]] = pkg("host.observe").observed_target_torch(case["depth"], case["labels"], OC.CHAN, OC.DCH, OC.NCH)
    return _YARDSTICK[case["name"]]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _builder(case):
    B, S, _ = case["depth"].shape
    return pkg("host.observe").ObservedTarget(OC.CHAN, OC.DCH, S, batch=B, device=DEV, nch=OC.NCH)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_torch_definition(case):
    ot = _builder(case)
    ot.target.fill_(float("nan")); ot.status.fill_(-1)
    target, status = ot(case["depth"].to(DEV), case["labels"].to(DEV))
    torch.cuda.synchronize()
    want, want_status = _yardstick(case)
    differ = torch.nonzero(_bits(target.cpu()) != _bits(want))
    assert differ.numel() == 0, "%d elements differ, planes %s" % (differ.shape[0], sorted(set(differ[:, 1].tolist())))
    assert torch.equal(status.cpu(), want_status)
    if case["status"] is not None:
        assert status.tolist() == case["status"]


def test_repeatable_and_capturable():
    case = [c for c in CASES if c["name"] == "mixed_s96_b3"][0]
    ot = _builder(case)
    d, l = case["depth"].to(DEV), case["labels"].to(DEV)
    first = [t.clone() for t in ot(d, l)]
    second = [t.clone() for t in ot(d, l)]
    assert torch.equal(_bits(first[0]), _bits(second[0])) and torch.equal(first[1], second[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                             # a linear capture: two kernel nodes
        ot(d, l)
    for _ in range(2):
        ot.target.fill_(7.0); ot.status.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(ot.target), _bits(first[0])) and torch.equal(ot.status, first[1])


def test_refusals_launch_nothing():
    OB, L = pkg("host.observe"), pkg("_lib")
    with pytest.raises(ValueError):
        OB.ObservedTarget(OC.CHAN, OC.DCH, 6, device=DEV)
    with pytest.raises(ValueError):
        OB.ObservedTarget(OC.CHAN, OC.DCH[:-1] + [-1], 12, device=DEV)
    case = [c for c in CASES if c["name"] == "absent_class_s12_b3"][0]
    B, S, _ = case["depth"].shape
    ot = _builder(case)
    ot.target.fill_(-7.0); ot.status.fill_(-5)
    d, l = case["depth"].to(DEV), case["labels"].to(DEV)
    for bad_d, bad_l in ((case["depth"], l), (d.double(), l), (d, l.to(torch.int32)), (d[:, :8].contiguous(), l), (d, l[:2].contiguous()), (d.half(), l)):
        with pytest.raises(ValueError):
            ot(bad_d, bad_l)
    # the C entry itself, every other argument valid
    lib, P, st = L.lib(), L.ptr, L.current_stream_ptr()
    i32 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int32))
    chan, dch = i32(OC.CHAN), i32(OC.DCH)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    off = lambda t, n: C.c_void_p(t.data_ptr() + n)
    big = torch.zeros(24, dtype=torch.float32, device=DEV)                      # a valid buffer behind the misaligned pointers below
    wide = torch.zeros(65 * 4, dtype=torch.int32).numpy()

    def call(depth=P(d), labels=P(l), B_=B, S_=S, NC=len(OC.CHAN), chan_=hp(chan), dch_=hp(dch), nch=OC.NCH, ws=P(ot._ws), out=P(ot.target),
             status=P(ot.status)):
        return lib.sln_observed_target(depth, labels, B_, S_, NC, chan_, dch_, nch, ws, out, status, st)
    unsupported = [dict(S_=6), dict(S_=0), dict(S_=4100), dict(B_=0), dict(B_=65536), dict(NC=0), dict(NC=65, chan_=hp(wide), dch_=hp(wide)),
                   dict(nch=69), dict(nch=71), dict(nch=73),
                   dict(dch_=hp(i32(OC.DCH[:-1] + [-1])))]                     # 28 owned channels under nch = 70
    for kw in unsupported:
        assert call(**kw) == -2, kw
    two = i32(OC.DCH); two[5] = two[4]
    low = i32(OC.DCH); low[1] = -2                                              # (a class without a depth channel: the count stays 29)
    high = i32(OC.DCH); high[3] = 29; high[4] = 29
    badarg = [dict(depth=None), dict(labels=None), dict(chan_=None), dict(dch_=None), dict(ws=None), dict(out=None), dict(status=None),
              dict(depth=off(big, 4)), dict(out=off(big, 8)), dict(labels=off(l, 1)), dict(status=off(ot.status, 2)), dict(ws=off(ot._ws, 2)),
              dict(chan_=hp(i32([40] + OC.CHAN[1:]))), dict(chan_=hp(i32([-1] + OC.CHAN[1:]))), dict(dch_=hp(two)), dict(dch_=hp(low)),
              dict(dch_=hp(high))]
    for kw in badarg:
        assert call(**kw) == -1, kw
    assert lib.sln_observed_target_workspace_bytes(B, 6) == -2 and lib.sln_observed_target_workspace_bytes(0, S) == -2
    assert lib.sln_observed_target_workspace_bytes(B, S) > 0
    torch.cuda.synchronize()
    assert bool((ot.target == -7.0).all()) and ot.status.tolist() == [-5] * B
    assert call() == 0                                                          # ... and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert torch.equal(_bits(ot.target.cpu()), _bits(_yardstick(case)[0]))


def test_round_trip_against_the_device_scene_pass():
    """Three random rooms rendered at S = 96 by RefineScene.render, observed, rebuilt.  Plane 0: equal.  Semantic planes: within
    32 * 2^-24 (the render's trilinear weights round ~17 times, the rebuilt planes are exactly 0 or 1).  Depth-hot planes: within 2^-23;
    both sides sum in the same fixed point, so equal bits are expected - the count of differing elements is printed (LAB_NOTES)."""
    from test_refine_gpu import FURN, _random_rooms
    R, OB = pkg("host.refine"), pkg("host.observe")
    cfg = vae_ref.VaeConfig()
    rooms = _random_rooms(3, cfg, seed=3)
    bank = R.MeshBank(FURN, DEV, seed=3)
    renders, scenes = [], []
    with torch.no_grad():
        for rm in rooms:
            sc = R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), 96)
            renders.append(sc.render(rm["boxes"], rm["angles"].float())[0]); scenes.append(sc)
    render = torch.cat(renders, 0)
    depth, labels = OB.observe(render)
    ot = OB.ObservedTarget(scenes[0].chan, scenes[0].dch, 96, batch=3, device=DEV)
    target, status = ot(depth, labels)
    torch.cuda.synchronize()
    reading = (depth > 0) & (depth <= 15)
    sem = float((target[:, 1:41] - render[:, 1:41]).abs().max())
    hot = target[:, 41:] != render[:, 41:]
    hot_max = float((target[:, 41:] - render[:, 41:]).abs().max())
    print("device round trip: status %s, pixels with a class but no reading %d, with a reading but no class %d, semantic max |diff| %.3g "
          "(%.1f x 2^-24), depth-hot: %d elements in %d (room, plane) pairs differ, max |diff| %.3g" % (
              status.tolist(), int(((labels > 0) & ~reading).sum()), int((reading & (labels == 0)).sum()), sem, sem * 2 ** 24,
              int(hot.sum()), int(hot.flatten(2).any(2).sum()), hot_max))
    assert torch.equal(target[:, 0], render[:, 0])
    assert sem <= 32 * 2.0 ** -24
    assert hot_max <= 2.0 ** -23
    assert status.tolist() == [0, 0, 0]
