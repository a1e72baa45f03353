"""Sg2ScVAEModel.gemm_precision on the device (run with -m gpu on an MI355X): the eval-mode encoder and decoder in the "f16x3" and
"f16" modes against the fp64 oracle, which launches take the fp16-MFMA route (sln_debug_vae_half_launches), and that everything
else - "fp32", training-mode forwards, train_step, RefineBatch - stays where it was.

Batch, seeds and configs are those of tools/vae_half_budget.py (its `inputs`).  Bounds: "f16x3" the project's 1e-4 per tensor
(tests/parity.py); "f16" twice the tool's committed CPU emulation of the same rounding (BUDGET), the rule of test_spade_f16_gpu.py."""
import importlib.util
import os
from unittest import mock

import numpy as np
import pytest
import torch

import parity
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

from oracle import vae_ref                                   # noqa: E402


def _tool():
    spec = importlib.util.spec_from_file_location("vae_half_budget", os.path.join(ROOT, "tools", "vae_half_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


B = _tool()
_cache = {}


def _case(name):
    """(cfg, state, batch, z, fp64 truth) of a budget config: computed once, never modified."""
    if name not in _cache:
        cfg, sd, batch, z = B.inputs(name)
        _cache[name] = (cfg, sd, batch, z, B.evaluate(cfg, sd, batch, z, None))
    return _cache[name]


def _model(cfg, sd):
    M = pkg("host.Sg2ScVAE_model")
    m = M.Sg2ScVAEModel(**cfg.model_kwargs())
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.cuda().eval()


def _dev(batch):
    return [t.cuda() for t in batch[:5]]


def _run(model, batch, z, encoder=True):
    objs, triples, boxes, angles, attrs = batch
    with torch.no_grad():
        bp, ap = model.decoder(z, objs, triples, attrs)
        out = dict(boxes=bp, angles=ap)
        if encoder:
            out["mu"], out["logvar"] = model.encoder(objs, triples, boxes, angles, attrs)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in out.items()}


def _half_count(model):
    return int(pkg("_lib").lib().sln_debug_vae_half_launches(model._eng))


@pytest.mark.parametrize("name", list(B.CONFIGS))
def test_half_modes_against_the_fp64_oracle(name):
    cfg, sd, batch, z, truth = _case(name)
    model = _model(cfg, sd)
    dev, zd = _dev(batch), z.cuda()
    model.gemm_precision = "f16x3"
    got = _run(model, dev, zd)
    for t in B.TENSORS:
        print("%s f16x3 %s: rel err %.3e" % (name, t, B.rel_err(got[t], truth[t])))
    for t in B.TENSORS:
        parity.assert_close(got[t].numpy(), truth[t].numpy(), "%s f16x3 %s" % (name, t))
    model.gemm_precision = "f16"
    got = _run(model, dev, zd)
    err = {t: B.rel_err(got[t], truth[t]) for t in B.TENSORS}
    print("%s f16: %s | budget %s" % (name, err, B.BUDGET[name]["f16"]))
    for t in B.TENSORS:
        assert np.isfinite(err[t]) and err[t] <= 2.0 * B.BUDGET[name]["f16"][t], "%s f16 %s: %.3e > 2 x %.3e" % (name, t, err[t], B.BUDGET[name]["f16"][t])


def test_only_eval_forwards_in_a_half_mode_take_the_route():
    cfg, sd, batch, z, _ = _case("default")
    model = _model(cfg, sd)
    dev, zd = _dev(batch), z.cuda()
    per_decode = 4 * cfg.gconv_num_layers + 2            # the four Linears of every GraphTripleConv, box_net.0 and angle_net.0
    _run(model, dev, zd, encoder=False)                  # creates the engine
    assert _half_count(model) == 0, "fp32 is the default and launches nothing on the fp16 route"
    for mode in ("f16x3", "f16"):
        model.gemm_precision = mode
        n0 = _half_count(model)
        _run(model, dev, zd, encoder=False)
        assert _half_count(model) - n0 == per_decode, (mode, _half_count(model) - n0, per_decode)
    n0 = _half_count(model)
    _run(model, dev, zd)                                 # the encoder's gconvs and the first two stages of both posterior heads as well
    assert _half_count(model) - n0 == per_decode + 4 * cfg.gconv_num_layers + 4
    model.gemm_precision = "fp32"
    n0 = _half_count(model)
    _run(model, dev, zd)
    assert _half_count(model) == n0
    model.gemm_precision = "f16x3"
    n0 = _half_count(model)
    model.train()
    with torch.no_grad():
        model(*dev, eps=zd)                              # a training-mode forward
    eps = zd
    model.train_step(*dev, kl_weight=0.1, lr=1e-4, eps=eps, use_graph=False)
    model.eval()
    model.train_step(*dev, kl_weight=0.1, lr=1e-4, eps=eps, use_graph=False)      # train.py:63-65: eval-mode BatchNorm, still training
    torch.cuda.synchronize()
    assert _half_count(model) == n0, "training-mode forwards and train_step stay on fp32"


def _rooms(n_rooms):
    """Small synthetic rooms in the form RefineBatch takes (as tests/test_hardening_gpu.py builds them)."""
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
        rooms.append(dict(objs=torch.tensor([3, 4, 6, 5, 7, 0]).cuda(), triples=tri.cuda(), boxes=boxes.cuda(),
                          angles=torch.randint(0, 24, (n,), generator=g).cuda(), attributes=torch.zeros(n, dtype=torch.int64, device="cuda"),
                          class_names=names))
    return rooms


def test_refine_batch_stays_fp32():
    """Recorded steps (room groups) never take the route, whatever the model's attribute and the room engines' own mode say."""
    H = pkg("_lib")
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=2)
    model = _model(cfg, vae_ref.init_state(cfg, seed=1))
    model.gemm_precision = "f16x3"
    rb = pkg("host.refine").RefineBatch(model, _rooms(2), image_size=96, iters=2)
    try:
        for e in rb._engines:
            H.check(H.lib().sln_vae_set_gemm_precision(e[0], 3), "sln_vae_set_gemm_precision")
        rb.run(1)
        torch.cuda.synchronize()
        assert [int(H.lib().sln_debug_vae_half_launches(e[0])) for e in rb._engines] == [0] * len(rb._engines)
        assert model._eng is None or _half_count(model) == 0
        assert H.lib().sln_vae_set_gemm_precision(rb._engines[0][0], 2) == -1       # not a mode
    finally:
        rb.close()
    assert model.gemm_precision == "f16x3"


def test_fp32_bits_come_back_after_a_half_mode():
    cfg, sd, batch, z, _ = _case("default")
    model = _model(cfg, sd)
    dev, zd = _dev(batch), z.cuda()
    first = _run(model, dev, zd)
    model.gemm_precision = "f16x3"
    half = _run(model, dev, zd)
    model.gemm_precision = "fp32"
    again = _run(model, dev, zd)
    for t in B.TENSORS:
        assert torch.equal(first[t], again[t]), t
    assert any(not torch.equal(first[t], half[t]) for t in B.TENSORS), "the half mode ran the fp32 launches"


def test_replicas_of_one_graph_decode_to_identical_rows():
    """A row's result does not depend on where it sits in the launch: 64 disjoint copies of one graph, fed the same z rows."""
    S = pkg("host.sampling")
    cfg, sd, _, _, _ = _case("default")
    model = _model(cfg, sd)
    objs, triples, _, _, attrs = vae_ref.synth_batch(1, B.OBJS, B.TRIPLES, seed=B.BATCH_SEED, cfg=cfg)[:5]
    n, O = 64, objs.shape[0]
    ro, rt, ra = S.replicate_graphs(objs.cuda(), triples.cuda(), attrs.cuda(), n)
    z = torch.randn(O, cfg.embedding_dim, generator=torch.Generator().manual_seed(3)).cuda().repeat(n, 1)
    for mode in ("f16x3", "f16"):
        model.gemm_precision = mode
        with torch.no_grad():
            bp, ap = model.decoder(z, ro, rt, ra)
        torch.cuda.synchronize()
        bp, ap = bp.view(n, O, -1).cpu(), ap.view(n, O, -1).cpu()
        assert bool(torch.isfinite(bp).all())
        assert bool((bp == bp[:1]).all()) and bool((ap == ap[:1]).all()), mode


def test_changed_parameters_are_read_afresh():
    """No packed copy of the weights exists: an in-place edit + params_changed() and a train_step both show in the next decode."""
    cfg, sd, batch, z, _ = _case("default")
    model = _model(cfg, sd)
    dev, zd = _dev(batch), z.cuda()
    model.gemm_precision = "f16x3"
    before = _run(model, dev, zd)
    key = "gconv_net_dc.gconvs.1.net1.0.weight"
    with torch.no_grad():
        dict(model.named_parameters())[key].mul_(1.5)            # a view of flat_params(): edited in place
    model.params_changed()

    def check(what):
        state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        truth = B.evaluate(cfg, state, batch, z, None)
        got = _run(model, dev, zd)
        for t in B.TENSORS:
            parity.assert_close(got[t].numpy(), truth[t].numpy(), "%s: f16x3 %s" % (what, t))
        return got
    scaled = check("after scaling " + key)
    assert float((scaled["boxes"] - before["boxes"]).abs().max()) > 1e-3 * float(before["boxes"].abs().max()), "the edit is not visible"
    model.train()
    model.train_step(*dev, kl_weight=0.1, lr=1e-3, eps=zd, use_graph=False)
    model.eval()
    stepped = check("after one train_step")
    assert not torch.equal(stepped["boxes"], scaled["boxes"])


def test_sample_layouts_precision_argument():
    S = pkg("host.sampling")
    cfg, sd, batch, _, _ = _case("default")
    model = _model(cfg, sd)
    objs, triples, _, _, attrs = _dev(vae_ref.synth_batch(1, B.OBJS, B.TRIPLES, seed=B.BATCH_SEED, cfg=cfg))
    gen = lambda: torch.Generator().manual_seed(9)               # noqa: E731
    b32, _, z32 = S.sample_layouts(model, objs, triples, attrs, n_samples=3, generator=gen(), precision="fp32")
    n0 = _half_count(model)
    model.gemm_precision = "f16"
    b3, _, z3 = S.sample_layouts(model, objs, triples, attrs, n_samples=3, generator=gen(), precision="f16x3")
    assert model.gemm_precision == "f16", "the previous mode comes back"
    assert _half_count(model) - n0 == 4 * cfg.gconv_num_layers + 2
    assert torch.equal(z3, z32)
    parity.assert_close(b3.cpu().numpy(), b32.cpu().numpy(), "sample_layouts f16x3 boxes against fp32")
    model.gemm_precision = "fp32"
    n0 = _half_count(model)
    S.sample_layouts(model, objs, triples, attrs, n_samples=3, generator=gen())          # None: the model's own setting
    assert _half_count(model) == n0
    with mock.patch.object(model, "decoder", side_effect=RuntimeError("decode failed")):
        with pytest.raises(RuntimeError):
            S.sample_layouts(model, objs, triples, attrs, n_samples=3, generator=gen(), precision="f16x3")
    assert model.gemm_precision == "fp32" and not model.training
    with pytest.raises(ValueError):
        S.sample_layouts(model, objs, triples, attrs, n_samples=3, generator=gen(), precision="bf16")
