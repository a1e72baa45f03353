"""RefineBatch(observed=...): the rooms' targets built from observed depth and label images (host/observe.py) instead of rendered from
the rooms' ground-truth boxes - routing, agreement with the default route on the rooms' own renders, room independence, the use case."""
import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import vae_ref
from test_refine_gpu import FURN, _random_rooms, _room_model

pytestmark = pytest.mark.gpu

S = 96
_SETUP = {}


def _setup():
    """model, three random rooms, the bank, the rooms' own renders and their observation - built once, never modified"""
    if not _SETUP:
        R, OB = pkg("host.refine"), pkg("host.observe")
        cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2, mlp_normalization="batch", use_attr=False)
        model, _ = _room_model(cfg)
        rooms = _random_rooms(3, cfg, seed=11)
        bank = R.MeshBank(FURN, "cuda", seed=3)
        with torch.no_grad():
            render = torch.cat([R.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), S).render(rm["boxes"], rm["angles"].float())[0]
                                for rm in rooms], 0)
        depth, labels = OB.observe(render)
        torch.cuda.synchronize()
        _SETUP.update(model=model, rooms=rooms, bank=bank, depth=depth, labels=labels,
                      kw=dict(bank=bank, learning_rate=1e-3, image_size=S, iters=4))
    return _SETUP


def test_observed_targets_are_routed_into_the_loss_and_the_pictures():
    R, OB = pkg("host.refine"), pkg("host.observe")
    s = _setup()
    rb = R.RefineBatch(s["model"], s["rooms"], observed=(s["depth"], s["labels"]), pictures="ends", **s["kw"])
    try:
        target, status = OB.ObservedTarget(rb.chan, rb.dch, S, batch=3)(s["depth"], s["labels"])
        rl = R.RefineLoss(target, per_room=True)
        torch.cuda.synchronize()
        assert torch.equal(rb.loss.target_depth.view(torch.int32), rl.target_depth.view(torch.int32))
        assert torch.equal(rb.loss.labels, rl.labels)
        assert torch.equal(rb.target_pictures.labels, s["labels"])
        assert torch.equal(rb.target_status, status) and rb.target_status.tolist() == [0, 0, 0]
        # against the default route on the same rooms: the targets rendered from the rooms' own boxes
        rb0 = R.RefineBatch(s["model"], s["rooms"], **s["kw"])
        try:
            assert rb0.target_status is None
            off = float((rb.loss.labels != rb0.loss.labels).float().mean())
            far = float((rb.loss.target_depth - rb0.loss.target_depth).abs().max())
            print("pooled labels that disagree: %.3g of the pixels; pooled target depths: max |diff| %.3g" % (off, far))
            assert off < 2e-3                                     # two resamplings of one target (test_refine_gpu.py: _torch_loss_and_gradient)
            assert far <= 2.0 ** -23
        finally:
            rb0.close()
    finally:
        rb.close()


def _state(rb, capture=False):
    losses = rb.run(capture=capture).cpu().numpy().copy()
    out = dict(losses=losses, boxes=[b.cpu().numpy().copy() for b, _ in rb.results()], z=rb.z.cpu().numpy().copy(),
               params=rb.params.cpu().numpy().copy(), row0=list(rb.row0), rows=list(rb.rows))
    rb.close()
    return out


def test_a_rooms_numbers_do_not_depend_on_the_other_rooms():
    """deterministic mode: R = 3 against each room alone with its own observation - losses, boxes, z and parameters bit-identical, eager
    and under a graph replay (as test_refine_gpu.py::test_rooms_in_flight_edge_cases holds the default route)"""
    R, L = pkg("host.refine"), pkg("_lib").lib()
    s = _setup()
    obs = lambda sel: (s["depth"][sel].contiguous(), s["labels"][sel].contiguous())
    try:
        L.sln_set_deterministic(1)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            full = _state(R.RefineBatch(s["model"], s["rooms"], observed=obs([0, 1, 2]), **s["kw"]))
            graph = _state(R.RefineBatch(s["model"], s["rooms"], observed=obs([0, 1, 2]), **s["kw"]), capture=True)
            ones = [_state(R.RefineBatch(s["model"], [s["rooms"][r]], observed=obs([r]), **s["kw"]), capture=(r == 0)) for r in range(3)]
        torch.cuda.synchronize()
    finally:
        L.sln_set_deterministic(0)
    assert np.isfinite(full["losses"]).all()
    for name, other, sel in [("graph", graph, [0, 1, 2])] + [("room %d alone" % r, ones[r], [r]) for r in range(3)]:
        for j, r in enumerate(sel):
            a, n, b = full["row0"][r], full["rows"][r], other["row0"][j]
            assert np.array_equal(other["losses"][:, j], full["losses"][:, r]), "%s: losses of room %d" % (name, r)
            assert np.array_equal(other["boxes"][j], full["boxes"][r]), "%s: boxes of room %d" % (name, r)
            assert np.array_equal(other["z"][b:b + n], full["z"][a:a + n]), "%s: z of room %d" % (name, r)
            assert np.array_equal(other["params"][j], full["params"][r]), "%s: parameters of room %d" % (name, r)


def test_refining_shifted_layouts_towards_an_observation():
    """the use case: the observations show the rooms' true boxes, the refinement starts from boxes shifted by +0.03 (room row kept)"""
    R = pkg("host.refine")
    s = _setup()
    moved = []
    for rm in s["rooms"]:
        b = rm["boxes"] + 0.03
        b[-1] = rm["boxes"][-1]
        moved.append(dict(rm, boxes=b))
    rb = R.RefineBatch(s["model"], moved, observed=(s["depth"], s["labels"]), **s["kw"])
    losses = rb.run().cpu().numpy().copy()
    rb.close()
    rb0 = R.RefineBatch(s["model"], s["rooms"], **s["kw"])
    default = rb0.run().cpu().numpy().copy()
    rb0.close()
    fell = lambda x: int(sum(x[-1, r] < x[0, r] for r in range(x.shape[1])))
    print("rooms whose loss fell over 4 iterations: %d of 3 towards the observation (shifted start), %d of 3 on the default route" % (
        fell(losses), fell(default)))
    print("losses towards the observation:\n%s\nlosses of the default route:\n%s" % (losses, default))
    assert np.isfinite(losses).all()
    changed = sum(len(set(losses[:, r].tolist())) > 1 for r in range(3))
    assert changed >= 2, "only %d of 3 rooms saw their loss change" % changed


def test_refused_arguments():
    R = pkg("host.refine")
    s = _setup()
    d, l = s["depth"], s["labels"]
    with pytest.raises(ValueError):
        R.RefineBatch(s["model"], s["rooms"], observed=(d, l), retrieve=True, **s["kw"])
    for bad in ((d[:2].contiguous(), l), (d, l[:, :48].contiguous()), (d.double(), l), (d, l.to(torch.int32)), (d.cpu(), l), (d, l.cpu()), (d,), d):
        with pytest.raises(ValueError):
            R.RefineBatch(s["model"], s["rooms"], observed=bad, **s["kw"])
