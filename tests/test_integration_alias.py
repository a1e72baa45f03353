"""the reference's OWN factory (build_dataset_model.build_model) constructs the HIP-backed model when
``models.graph`` / ``models.Sg2ScVAE_model`` / ``data.suncg_dataset`` are aliased, with the reference model's parameter names and
shapes.  What the factory does was recorded from the reference by oracle/gen_golden_integration.py into
tests/golden/integration_layout.json: the names it imports from the aliased modules, the keyword arguments it hands the model
class, and the state_dict layout / parameter order of the reference classes built from them.  The HIP classes are held to that."""
import importlib
import json
import os
import types

import pytest
import torch

from conftest import GOLDEN

HOST = "3d_sln_amd.host."
ALIASES = {"models.graph": "graph", "models.Sg2ScVAE_model": "Sg2ScVAE_model", "data.suncg_dataset": "suncg_dataset"}


def _layout(module):
    return {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()}


def _synthetic_checkpoint(rec, seed):
    """a checkpoint with the reference's layout (keys, shapes, dtypes as recorded) and seeded contents"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, (shape, dtype) in rec["state_dict"].items():
        dt = getattr(torch, dtype)
        out[k] = torch.randn(shape, generator=g).to(dt) if dt.is_floating_point else torch.randint(0, 7, shape, generator=g).to(dt)
    return out


@pytest.fixture(scope="module")
def rec():
    with open(os.path.join(GOLDEN, "integration_layout.json")) as fh:
        return json.load(fh)


def test_reference_factory_builds_the_aliased_model(rec):
    mods = {name: importlib.import_module(HOST + m) for name, m in ALIASES.items()}
    for module, names in rec["factory_imports"].items():          # what `from <alias> import ...` in the factory needs
        assert module in mods, module
        for n in names:
            assert hasattr(mods[module], n), (module, n)
    # build_model's body on the recorded arguments: Sg2ScVAEModel(**kwargs), vocab passed through
    vocab = importlib.import_module(HOST + "synthetic").default_vocab()
    kwargs = dict(rec["model_kwargs"], vocab=vocab)
    assert {k: v for k, v in rec["factory_args"].items() if k in kwargs} == rec["model_kwargs"]
    model = mods["models.Sg2ScVAE_model"].Sg2ScVAEModel(**kwargs)
    assert type(model).__module__.startswith("3d_sln_amd.host"), type(model)
    a, b = _layout(model), rec["vae"]["state_dict"]
    assert a == b, sorted(set(map(str, a.items())) ^ set(map(str, b.items())))[:10]
    assert [n for n, _ in model.named_parameters()] == rec["vae"]["parameters"]      # optimizer state is positional
    ck = _synthetic_checkpoint(rec["vae"], 1)
    model.load_state_dict(ck)                                      # a reference checkpoint loads unchanged
    got = model.state_dict()
    assert all(torch.equal(got[k].cpu(), v) for k, v in ck.items())
    torch.optim.Adam(model.parameters(), lr=1e-4)
    n_params = sum(p.numel() for p in model.parameters())
    assert n_params == rec["vae"]["n_params"] == 3879790 and len(a) > 200
    # C. the generator, constructed as testing/test_SPADE_shade.py:9 does, small width to keep the test light
    g_hip = importlib.import_module(HOST + "SPADE_related").SPADEGenerator4(*rec["spade_args"])
    ga, gb = _layout(g_hip), rec["spade"]["state_dict"]
    assert ga == gb, sorted(set(map(str, ga.items())) ^ set(map(str, gb.items())))[:10]
    g_hip.load_state_dict(_synthetic_checkpoint(rec["spade"], 2))
    assert len(ga) == 230                                          # the 230-key checkpoint layout
