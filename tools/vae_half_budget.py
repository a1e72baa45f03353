"""CPU error budget of the VAE's half-precision modes (Sg2ScVAEModel.gemm_precision): the eval-mode encoder and decoder of the fp64
oracle (oracle/vae_ref.py) with the operands of every Linear that the HIP path routes to the fp16-MFMA kernel (csrc/gemm_half.hip:
outputs % 32 == 0, inputs % 16 == 0 - the GraphTripleConv Linears, box_net.0, angle_net.0 and the first two stages of the posterior
heads; not box_net.1, angle_net.1, the mu / logvar heads or box_embeddings) rounded as the kernel rounds them, against plain fp64:
    fp32   the oracle as it stands, in float32 (what the reference delivers)
    f16x3  hi = fp16(v), lo = fp16(v - hi) of the fp32 operands, a_hi w_lo + a_lo w_hi + a_hi w_hi
    f16    fp16(v) of the fp32 operands, one product
Products and sums of the two half modes stay fp64: the table isolates the operand rounding.  Printed per config and tensor:
max |err| / max |fp64 tensor| (the reading of tests/parity.py).

Inputs (tests/test_vae_half_gpu.py builds the same): vae_ref.synth_batch(8 graphs, 8 objects, 12 triples, seed=BATCH_SEED),
vae_ref.init_state(cfg, seed=STATE_SEED) - its running means ~ N(0, 0.1^2) and running variances ~ U(0.5, 1.5) are the perturbed
statistics of a trained model -, the decoder's z ~ N(0, 1) from numpy's default_rng(Z_SEED).

    python tools/vae_half_budget.py [--write]
BUDGET below is this tool's own output (--write rewrites it in place), every figure rounded to float32 so that a regeneration
reproduces it bit for bit whatever the BLAS does to the last bits of an fp64 sum; tests/test_vae_half_gpu.py bounds the GPU's
"f16" mode by 2x it."""
import argparse
import contextlib
import os
import re
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vae_ref                          # noqa: E402

MODES = ("fp32", "f16x3", "f16")
TENSORS = ("boxes", "angles", "mu", "logvar")
GRAPHS, OBJS, TRIPLES = 8, 8, 12
STATE_SEED, BATCH_SEED, Z_SEED = 42, 5, 11
CONFIGS = {                                         # VaeConfig overrides; "default" is train.py's
    "default": {},
    "no_decoder_cat": dict(decoder_cat=False),
    "recurrent": dict(gconv_mode="recurrent"),
    "no_norm": dict(mlp_normalization="none"),
    "no_attr": dict(use_attr=False),
}
# BUDGET-BEGIN (python tools/vae_half_budget.py --write)
BUDGET = {
    'default': {
        'fp32': {'boxes': 1.0995847787853563e-06, 'angles': 8.716007755538158e-07, 'mu': 7.963908501551487e-07, 'logvar': 7.931193408694526e-07},
        'f16x3': {'boxes': 7.564771067336551e-07, 'angles': 7.946136406644655e-07, 'mu': 9.580207915860228e-07, 'logvar': 1.302673808822874e-06},
        'f16': {'boxes': 0.0013783209724351764, 'angles': 0.0012968515511602163, 'mu': 0.0011110315099358559, 'logvar': 0.0012717065401375294},
    },
    'no_decoder_cat': {
        'fp32': {'boxes': 1.4134880075289402e-06, 'angles': 7.252087925735395e-07, 'mu': 1.1057657047786051e-06, 'logvar': 1.129502493313339e-06},
        'f16x3': {'boxes': 1.0450168019815465e-06, 'angles': 8.821472192721558e-07, 'mu': 1.465219838792109e-06, 'logvar': 1.7062022834579693e-06},
        'f16': {'boxes': 0.0017801456851884723, 'angles': 0.001197564764879644, 'mu': 0.0013441381743177772, 'logvar': 0.001640195376239717},
    },
    'recurrent': {
        'fp32': {'boxes': 6.889569590384781e-07, 'angles': 9.322883443019236e-07, 'mu': 9.134960805567971e-07, 'logvar': 9.660794830779196e-07},
        'f16x3': {'boxes': 6.070855533835129e-07, 'angles': 7.814443847564689e-07, 'mu': 1.062520595951355e-06, 'logvar': 9.322125720245822e-07},
        'f16': {'boxes': 0.0009297998039983213, 'angles': 0.0011656391434371471, 'mu': 0.0012743237894028425, 'logvar': 0.0013481378555297852},
    },
    'no_norm': {
        'fp32': {'boxes': 6.868393711556564e-07, 'angles': 3.936952737149113e-07, 'mu': 7.979896849974466e-07, 'logvar': 8.924689041123202e-07},
        'f16x3': {'boxes': 6.077406737858837e-07, 'angles': 4.070240606779407e-07, 'mu': 8.870392775861546e-07, 'logvar': 7.319782184822543e-07},
        'f16': {'boxes': 0.0009941324824467301, 'angles': 0.0005979437846690416, 'mu': 0.001401625107973814, 'logvar': 0.0010512513108551502},
    },
    'no_attr': {
        'fp32': {'boxes': 7.731874234195857e-07, 'angles': 8.157211937032116e-07, 'mu': 1.0298438155587064e-06, 'logvar': 8.891080369721749e-07},
        'f16x3': {'boxes': 8.062093570515572e-07, 'angles': 5.134198204359564e-07, 'mu': 1.044565692609467e-06, 'logvar': 8.879474648892938e-07},
        'f16': {'boxes': 0.001166956266388297, 'angles': 0.0007364703924395144, 'mu': 0.001545070786960423, 'logvar': 0.0014702673070132732},
    },
}
# BUDGET-END


def takes(n_out, n_in):
    """The shape part of the kernel's route predicate (sln_nt_half_takes); segment widths are multiples of 16 wherever K is."""
    return n_out % 32 == 0 and n_in % 16 == 0


def _f16(t):
    return t.clamp(-65504.0, 65504.0).half().double()


def rounded_linear(mode):
    """F.linear with the operands of the routed Linears rounded per `mode` (inputs fp64; the rest passes through)."""
    def f(x, w, b=None):
        if not takes(w.shape[0], w.shape[1]):
            return F.linear(x, w, b)
        x32, w32 = x.float().double(), w.float().double()
        xh, wh = _f16(x32), _f16(w32)
        if mode == "f16":
            return F.linear(xh, wh, b)
        xl, wl = _f16(x32 - xh), _f16(w32 - wh)
        return F.linear(xh, wl) + F.linear(xl, wh) + F.linear(xh, wh, b)
    return f


@contextlib.contextmanager
def patched_oracle(mode):
    """The oracle's F.linear replaced by rounded_linear(mode) (the oracle module's own `F` name only)."""
    class _FP:
        def __getattr__(self, n):
            return getattr(F, n)
    proxy = _FP()
    proxy.linear = rounded_linear(mode)
    old = vae_ref.F
    vae_ref.F = proxy
    try:
        yield
    finally:
        vae_ref.F = old


def inputs(name):
    """-> (cfg, state, batch, z): what every mode and the GPU test evaluate for config `name`."""
    cfg = vae_ref.VaeConfig(**CONFIGS[name])
    sd = vae_ref.init_state(cfg, seed=STATE_SEED)
    batch = vae_ref.synth_batch(GRAPHS, OBJS, TRIPLES, seed=BATCH_SEED, cfg=cfg)
    z = torch.from_numpy(np.random.default_rng(Z_SEED).standard_normal((batch[0].shape[0], cfg.embedding_dim)).astype(np.float32))
    return cfg, sd, batch, z


def evaluate(cfg, sd, batch, z, mode):
    """Eval-mode decoder(z) and encoder of the oracle -> {tensor: fp64}.  mode None: plain fp64; "fp32": the oracle in float32."""
    dt = torch.float32 if mode == "fp32" else torch.float64
    s = {k: (v.detach().to(dt) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    objs, triples, boxes, angles, attrs = batch[:5]
    ctx = patched_oracle(mode) if mode in ("f16x3", "f16") else contextlib.nullcontext()
    with torch.no_grad(), ctx:
        bp, ap = vae_ref.decoder(s, cfg, z.to(dt), objs, triples, attrs, False)
        mu, lv = vae_ref.encoder(s, cfg, objs, triples, boxes.to(dt), angles, attrs, False)
    return dict(boxes=bp.double(), angles=ap.double(), mu=mu.double(), logvar=lv.double())


def rel_err(got, truth):
    """max |got - truth| / max |truth|, rounded to float32 (see the module docstring)."""
    return float(np.float32(float((got.double() - truth).abs().max()) / max(float(truth.abs().max()), 1e-30)))


def budget(name):
    """-> {mode: {tensor: relative error against fp64}} for one config."""
    cfg, sd, batch, z = inputs(name)
    truth = evaluate(cfg, sd, batch, z, None)
    return {m: {t: rel_err(v, truth[t]) for t, v in evaluate(cfg, sd, batch, z, m).items()} for m in MODES}


def _write(table):
    lines = ["BUDGET = {"]
    for name in CONFIGS:
        lines.append("    %r: {" % name)
        for m in MODES:
            lines.append("        %r: {%s}," % (m, ", ".join("%r: %r" % (t, table[name][m][t]) for t in TENSORS)))
        lines.append("    },")
    lines.append("}")
    path = os.path.abspath(__file__)
    src = open(path).read()
    new = re.sub(r"(# BUDGET-BEGIN[^\n]*\n).*?(# BUDGET-END)", lambda mo: mo.group(1) + "\n".join(lines) + "\n" + mo.group(2), src, count=1,
                 flags=re.S)
    with open(path, "w") as fh:
        fh.write(new)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="rewrite the BUDGET dict of this file from this run")
    a = ap.parse_args()
    table = {}
    print("batch: %d graphs x %d objects x %d triples; relative error against fp64" % (GRAPHS, OBJS, TRIPLES))
    print("%-16s %-6s %s" % ("config", "mode", " ".join("%10s" % t for t in TENSORS)))
    for name in CONFIGS:
        table[name] = budget(name)
        for m in MODES:
            print("%-16s %-6s %s" % (name, m, " ".join("%10.2e" % table[name][m][t] for t in TENSORS)))
    if a.write:
        _write(table)
        print("BUDGET rewritten")
    elif table != BUDGET:
        print("note: this run differs from the committed BUDGET")


if __name__ == "__main__":
    main()
