"""Generate tests/golden/integration_layout.json by running the REFERENCE's own model factory on CPU.

Runs ONLY in the build container (needs /root/reference, read-only).  INTEGRATION.md section 2: with ``models.graph`` /
``models.Sg2ScVAE_model`` / ``data.suncg_dataset`` aliased to the HIP host modules, the reference's
``build_dataset_model.build_model`` constructs the HIP-backed model.  What that check needs from the reference is recorded here
as data: the names the factory imports from the aliased modules, the keyword arguments it hands the model class, the
state_dict layout (key -> shape, dtype) and parameter order of the reference ``Sg2ScVAEModel`` built from them, and the layout
of the reference ``SPADEGenerator4`` at the test's small width.  tests/test_integration_alias.py compares the HIP classes with
it.  Only data is written; no reference source travels.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_integration.py
"""
from __future__ import annotations

import ast
import importlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "integration_layout.json")
sys.dont_write_bytecode = True

# the test's factory arguments (options.py defaults at train.py's widths) and SPADE constructor arguments
# (testing/test_SPADE_shade.py:9, small width to keep the test light)
ARGS = dict(batch_size=64, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode="feedforward", gconv_num_layers=5,
            mlp_normalization="batch", vec_noise_dim=0, layout_noise_dim=32, use_AE=False, multigpu=False)
SPADE_ARGS = [41, 3, 16, 8, "spectralspadelayer3x3", 64, "normal"]


def layout(module):
    return {"state_dict": {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()},
            "parameters": [n for n, _ in module.named_parameters()],
            "n_params": int(sum(p.numel() for p in module.parameters()))}


def factory_imports(path):
    """{module: [names]} of the ``from X import a, b`` statements of the factory's source (the names an alias must provide)"""
    tree = ast.parse(open(path).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] in ("models", "data"):
            out.setdefault(node.module, []).extend(a.name for a in node.names)
    return out


def main():
    sys.path.insert(0, REF)
    sys.path.insert(0, ROOT)
    import torch
    ref_vae = importlib.import_module("models.Sg2ScVAE_model")
    ref_spade = importlib.import_module("models.SPADE_related")
    B = importlib.import_module("build_dataset_model")           # the reference's factory, on the reference's own modules
    vocab = importlib.import_module("3d_sln_amd.host.synthetic").default_vocab()
    torch.manual_seed(0)
    model, kwargs = B.build_model(types.SimpleNamespace(**ARGS), vocab)
    assert type(model) is ref_vae.Sg2ScVAEModel
    rec = {"about": "the reference's build_dataset_model.build_model on the test's arguments (oracle/gen_golden_integration.py)",
           "factory_imports": factory_imports(os.path.join(REF, "build_dataset_model.py")),
           "factory_args": ARGS,
           "model_kwargs": {k: v for k, v in kwargs.items() if k != "vocab"},
           "model_kwargs_vocab": "the vocab handed to build_model, passed through unchanged",
           "vae": layout(model),
           "spade_args": SPADE_ARGS,
           "spade": layout(ref_spade.SPADEGenerator4(*SPADE_ARGS))}
    assert kwargs["vocab"] is vocab
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=False)
        fh.write("\n")
    print("wrote %s: %d VAE keys, %d parameters; %d SPADE keys" % (os.path.relpath(OUT, ROOT), len(rec["vae"]["state_dict"]),
                                                                   rec["vae"]["n_params"], len(rec["spade"]["state_dict"])))


if __name__ == "__main__":
    main()
