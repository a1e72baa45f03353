"""CPU tests of the VAE's opt-in fp16-MFMA precision modes: the route predicate of csrc/gemm_half.hip (host only, through
sln_debug_gemm_nt_half_takes on descriptions with placeholder addresses), the Sg2ScVAEModel.gemm_precision switch on a CPU-resident
model, and the emulated error budget (tools/vae_half_budget.py)."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

import gemm_cases as GC
import gemm_ref as R
import parity
from conftest import ROOT, pkg

from oracle import vae_ref                         # noqa: E402


def _budget():
    spec = importlib.util.spec_from_file_location("vae_half_budget", os.path.join(ROOT, "tools", "vae_half_budget.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _problem(key, M, N, K, lens, mode, epi=R.EPI_PLAIN, variant=0, **over):
    kw = dict(addend=None, ycol0=4, ldy=N + 12)
    kw.update(over)
    return GC.nt_problem(key, M, N, K, lens, mode, epi, -1, variant).replace(**kw)


def _takes(p):
    L = pkg("_lib")
    d = GC.nt_desc(L, p, GC.fake_ptr, Y=1, osums=1)
    return L.lib().sln_debug_gemm_nt_half_takes(C.byref(d))


# the decoder's Linears at train.py's sizes (E = 64, H = 256), and one MFMA step with a ragged row count
TAKEN = [
    ("net1.0", 200, 256, 384, (128, 128, 128), "affine"),
    ("net1.1", 133, 640, 256, None, "affine"),
    ("net2.0", 70, 256, 256, None, "ident"),
    ("net2.1", 300, 128, 256, None, "affine"),
    ("box_net.0", 70, 256, 144, (128, 16), "affine"),
    ("angle_net.0", 70, 256, 128, None, "affine"),
    ("one-step", 33, 32, 16, None, "ident"),
]


@pytest.mark.parametrize("case", TAKEN, ids=[c[0] for c in TAKEN])
def test_predicate_takes(case):
    name, M, N, K, lens, mode = case
    for bias in (True, False):
        p = _problem("takes-" + name, M, N, K, lens, mode)
        assert _takes(p if bias else p.replace(bias=None)) == 1
    assert _takes(_problem("takes-" + name, 1, N, K, lens, mode)) == 1          # M plays no part


REFUSED = [
    ("N=6", dict(M=70, N=6, K=256, lens=None, mode="affine")),
    ("N=24", dict(M=70, N=24, K=256, lens=None, mode="affine")),
    ("K=36", dict(M=70, N=64, K=36, lens=None, mode="ident")),
    ("concat-36|100", dict(M=133, N=64, K=136, lens=(36, 100), mode="ident")),
    ("two-source", dict(M=70, N=64, K=256, lens=None, mode="bwd")),
    ("stats", dict(M=70, N=64, K=256, lens=None, mode="affine", epi=R.EPI_STATS)),
    ("mask", dict(M=70, N=64, K=256, lens=None, mode="affine", epi=R.EPI_MASK)),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_predicate_refuses(case):
    name, kw = case
    p = _problem("refuse-" + name, kw["M"], kw["N"], kw["K"], kw["lens"], kw["mode"], kw.get("epi", R.EPI_PLAIN))
    assert _takes(p) == 0


def test_predicate_refuses_an_addend_and_an_unaligned_window():
    base = _problem("refuse-window", 70, 64, 256, None, "affine")
    assert _takes(base) == 1
    full = GC.nt_problem("refuse-window", 70, 64, 256, None, "affine", R.EPI_PLAIN, -1, 0)
    assert _takes(full.replace(ycol0=4, ldy=76)) == 0                             # its addend is still there
    assert _takes(base.replace(ycol0=3, ldy=76)) == 0
    assert _takes(base.replace(ycol0=4, ldy=74)) == 0
    L = pkg("_lib")
    d = GC.nt_desc(L, base, GC.fake_ptr, Y=1, osums=1)
    d.K = 40                                                                      # a malformed description is an error, not a refusal
    assert L.lib().sln_debug_gemm_nt_half_takes(C.byref(d)) == -1
    assert L.lib().sln_debug_gemm_nt_half_takes(None) == -1


def test_gemm_precision_on_a_cpu_model():
    M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=1)
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    assert model.gemm_precision == "fp32"
    for mode in ("f16x3", "f16", "fp32"):
        model.gemm_precision = mode
        assert model.gemm_precision == mode
    model.gemm_precision = "f16x3"
    for bad in ("bf16", "FP32", None, 3):
        with pytest.raises(ValueError):
            model.gemm_precision = bad
    assert model.gemm_precision == "f16x3"                                        # a refused value changes nothing
    assert not any("precision" in k for k in model.state_dict())
    other = M.Sg2ScVAEModel(**cfg.model_kwargs())
    other.load_state_dict(model.state_dict())
    assert other.gemm_precision == "fp32"


def test_emulated_budget_of_the_default_config():
    """f16x3 stays fp32-grade through the whole eval decoder and encoder (the project's 1e-4 bar, tests/parity.py's reading); the f16
    figures regenerate the committed BUDGET bit for bit."""
    B = _budget()
    cfg, sd, batch, z = B.inputs("default")
    truth = B.evaluate(cfg, sd, batch, z, None)
    x3 = B.evaluate(cfg, sd, batch, z, "f16x3")
    for t in B.TENSORS:
        parity.assert_close(x3[t].numpy(), truth[t].numpy(), "f16x3 " + t)
    x1 = B.evaluate(cfg, sd, batch, z, "f16")
    got = {t: B.rel_err(x1[t], truth[t]) for t in B.TENSORS}
    assert got == B.BUDGET["default"]["f16"], (got, B.BUDGET["default"]["f16"])
    assert set(B.BUDGET) == set(B.CONFIGS) and all(set(B.BUDGET[c]) == set(B.MODES) for c in B.BUDGET)
    assert min(got.values()) > 100 * max(B.rel_err(x3[t], truth[t]) for t in B.TENSORS)      # the one-product mode really rounds
