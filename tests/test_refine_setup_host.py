"""The set-up pieces the three refinement loops share (host/refine.py), the parts that need no GPU: the iteration-schedule parser of
``report`` / ``pictures``, the cut of the SGD ranges around the tensors the wgrad launches step themselves, a room's start (z draw and
noise rows on one seeded CPU generator) and the ``observed=`` argument check."""
import types

import pytest
import torch

from conftest import pkg


# ------------------------------------------------------------------------------------------------------------------------------
# parse_schedule
# ------------------------------------------------------------------------------------------------------------------------------
def test_schedule_of_four_iterations():
    R = pkg("host.refine")
    assert R.parse_schedule("all", 4, "report") == ((0, 1, 2, 3), True)
    assert R.parse_schedule("ends", 4, "report") == ((0, 3), False)
    assert R.parse_schedule([2, 2, 1], 4, "report") == ((1, 2), False)
    assert R.parse_schedule(iter([3, 0]), 4, "pictures") == ((0, 3), False)
    assert R.parse_schedule(None, 4, "report") is None
    for bad in ("some", [7], [-1], [4]):
        with pytest.raises(ValueError) as e:
            R.parse_schedule(bad, 4, "pictures")
        assert "pictures" in str(e.value)


@pytest.mark.parametrize("iters", [1, 0])
def test_schedule_of_one_and_of_no_iteration(iters):
    R = pkg("host.refine")
    assert R.parse_schedule("ends", iters, "report") == ((0,), False)
    assert R.parse_schedule("all", iters, "report") == ((0,), True)          # iters = 0: a row nothing consults
    assert R.parse_schedule([0], iters, "report") == ((0,), False)
    with pytest.raises(ValueError):
        R.parse_schedule([1], iters, "report")


# ------------------------------------------------------------------------------------------------------------------------------
# cut_ranges (the values: computed with the interval arithmetic as it stood inside RefineBatch.__init__)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranges,offsets,lengths,want", [
    ([(0, 1024)], [64, 512], [100, 64], [(0, 64), (192, 320), (576, 448)]),           # every offset on 64: lengths padded to 64
    ([(0, 256), (512, 256)], [0, 640], [256, 128], [(512, 128)]),                     # a run cut away whole, a hole inside the next
    ([(0, 256)], [4, 100], [8, 10], [(0, 4), (12, 88), (112, 144)]),                  # offsets off 64: lengths padded to 4
    ([(0, 1024)], [512, 64], [64, 100], [(0, 64), (192, 320), (576, 448)]),           # (the cuts in any order)
    ([(0, 256)], None, None, [(0, 256)]),
    ([(0, 256)], [], [], [(0, 256)]),
])
def test_cut_ranges(ranges, offsets, lengths, want):
    R = pkg("host.refine")
    assert R.cut_ranges(ranges, offsets, lengths) == want
    assert ranges == [tuple(r) for r in ranges]                                       # (the argument is left alone)


@pytest.mark.parametrize("ranges,offsets,lengths", [
    ([(64, 256)], [0], [128]),                    # starts before the run it reaches into
    ([(0, 256)], [6], [8]),                       # not on a multiple of 4 floats
    ([(0, 256)], [8, 12], [8, 8]),                # starts before the position the cut in front of it reached (8 + 8)
])
def test_cut_ranges_refuses(ranges, offsets, lengths):
    R, Lm = pkg("host.refine"), pkg("_lib")
    with pytest.raises(Lm.SlnError):
        R.cut_ranges(ranges, offsets, lengths)


# ------------------------------------------------------------------------------------------------------------------------------
# room_start
# ------------------------------------------------------------------------------------------------------------------------------
class _StubModel:
    """an encoder that returns fixed ``mu`` / ``logvar`` and notes what it was called with, in which precision"""

    def __init__(self, n=5, E=3):
        g = torch.Generator().manual_seed(99)
        self.mu, self.logvar = torch.randn(n, E, generator=g), torch.randn(n, E, generator=g) * 0.3
        self.gemm_precision, self.seen = "bf16x3", []

    def encoder(self, objs, triples, boxes, angles, attributes):
        self.seen.append(("encoder", self.gemm_precision, (objs, triples, boxes, angles, attributes)))
        return self.mu, self.logvar


ROOM = dict(objs="o", triples="t", boxes="b", angles="a", attributes="x")


@pytest.mark.parametrize("iters", [0, 3])
def test_room_start_draws_z_then_one_noise_row_per_iteration(iters):
    R = pkg("host.refine")
    model = _StubModel()
    z0, noise = R.room_start(model, ROOM, 13, iters, "cpu")
    gen = torch.Generator(device="cpu").manual_seed(13)
    want_z = model.mu + torch.randn(model.mu.shape, generator=gen) * torch.exp(0.5 * model.logvar)
    want_noise = [torch.randn(5, generator=gen) for _ in range(iters)]
    assert torch.equal(z0, want_z) and not z0.requires_grad
    assert noise.shape == (iters, 5) and noise.dtype == torch.float32 and noise.device.type == "cpu"
    for k in range(iters):
        assert torch.equal(noise[k], want_noise[k]), k
    # one encoder call: the room's five tensors in the encoder's order, the model's own precision
    assert model.seen == [("encoder", "bf16x3", ("o", "t", "b", "a", "x"))]
    again = R.room_start(_StubModel(), ROOM, 13, iters, "cpu")
    assert torch.equal(again[0], z0) and torch.equal(again[1], noise)
    other = R.room_start(_StubModel(), ROOM, 14, iters, "cpu")
    assert not torch.equal(other[0], z0)


def test_room_start_fp32_holds_for_the_encoder_call_only():
    R = pkg("host.refine")
    model = _StubModel()
    z0, _ = R.room_start(model, ROOM, 13, 2, "cpu", fp32=True)
    assert model.seen[0][1] == "fp32" and model.gemm_precision == "bf16x3"
    assert torch.equal(z0, R.room_start(_StubModel(), ROOM, 13, 2, "cpu")[0])


# ------------------------------------------------------------------------------------------------------------------------------
# check_observed
# ------------------------------------------------------------------------------------------------------------------------------
def test_check_observed():
    R = pkg("host.refine")
    d, l = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8)
    cpu = torch.device("cpu")
    R.check_observed(None, (2, 8, 8), cpu, cuda=False)
    R.check_observed(None, (2, 8, 8), cpu, cuda=True)
    R.check_observed((d, l), (2, 8, 8), cpu, cuda=False)
    R.check_observed([d.double(), l], (2, 8, 8), cpu, cuda=False)              # the torch route takes any depth dtype
    # what both routes refuse: no pair of tensors, another shape, labels that are not uint8, another device
    bad = [d, (d,), (d, l, l), (d, None), (d.numpy(), l), (d[:1], l), (d, l[:, :4]), (d, l.to(torch.int32)), (d, l.float())]
    for cuda in (False, True):
        for b in bad:
            with pytest.raises(ValueError):
                R.check_observed(b, (2, 8, 8), cpu, cuda=cuda)
    with pytest.raises(ValueError):
        R.check_observed((d, l), (2, 8, 8), torch.device("meta"), cuda=False)
    # a choice of meshes (retrieve=True, a bank that leaves one) combines with no observation at all
    R.check_observed(None, (2, 8, 8), cpu, cuda=False, choice=True)
    with pytest.raises(ValueError, match="no meshes to retrieve"):
        R.check_observed((d, l), (2, 8, 8), cpu, cuda=False, choice=True)
    # the device route: float32 depth on a GPU (ObservedTarget's own check) - host tensors never pass
    for b in ((d, l), (d.double(), l)):
        with pytest.raises(ValueError):
            R.check_observed(b, (2, 8, 8), cpu, cuda=True)


def test_one_room_arguments_lift_and_refuse():
    R = pkg("host.refine")
    d, l, m = torch.zeros(8, 8), torch.zeros(8, 8, dtype=torch.uint8), torch.ones(8, 8, dtype=torch.bool)
    cpu = torch.device("cpu")
    obs, mask = R._one_room_arguments((d, l), m, 8, cpu, cuda=False)
    assert [tuple(t.shape) for t in obs] == [(1, 8, 8)] * 2 and tuple(mask.shape) == (1, 8, 8)
    obs, mask = R._one_room_arguments((d[None], l[None]), "readings", 8, cpu, cuda=False)
    assert [tuple(t.shape) for t in obs] == [(1, 8, 8)] * 2 and mask == "readings"
    assert R._one_room_arguments(None, None, 8, cpu, cuda=False) == (None, None)
    for bad in (d, (d,), (d, l[:4]), (d, l.float())):
        with pytest.raises(ValueError):
            R._one_room_arguments(bad, None, 8, cpu, cuda=False)
    with pytest.raises(ValueError):
        R._one_room_arguments(None, "readings", 8, cpu, cuda=False)             # 'readings' needs observed
    # the loops refuse before they touch the model: None stands in for it
    args = (None, None, None, torch.zeros(2, 6), None, None, ["bed", "__room__"])
    with pytest.raises(ValueError):
        R.finetune_vae(*args, image_size=8, observed=(d, l.float()))
    bank = types.SimpleNamespace(has_choice=lambda: True)
    with pytest.raises(ValueError):
        R.finetune_vae(*args, image_size=8, observed=(d, l), bank=bank)         # observed with a bank that leaves a choice
