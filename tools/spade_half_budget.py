"""CPU error budget of the half-precision conv modes (SPADEGenerator4.conv_precision): the fp64 oracle (oracle/spade_ref.py) with the
operands of every 3x3 convolution that the HIP path routes to the fp16 kernel (mlp_shared, mlp_gamma, mlp_beta, conv_0, conv_1;
not the one-channel depth pre-conv, conv_s or conv_img) rounded as the kernel rounds them, against the plain fp64 evaluation:
    fp32   operands rounded to fp32 (what the fp32 kernel multiplies)
    f16x3  hi = fp16(v), lo = fp16(v - hi) of the fp32 operands, x_hi w_hi + x_lo w_hi + x_hi w_lo
    f16    fp16(v) of the fp32 operands, one product
Products and sums stay fp64: the table isolates the operand rounding.  Printed per weight set: max |err| / scale, mean |err|, the
share of save_color bytes that differ from the fp64 image's and the largest byte difference; then max |operand| per conv and the
share of nonzero lo parts that are fp16-subnormal.
    python tools/spade_half_budget.py [--small] [--sets bench,oracle]
BUDGET below is this tool's output at full size (256 x 256, ngf 64, batch 1); tests/test_spade_f16_gpu.py bounds the GPU by 2x it."""
import argparse
import contextlib
import importlib
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import spade_ref                        # noqa: E402

MODES = ("fp32", "f16x3", "f16")
BUDGET = {                                # python tools/spade_half_budget.py --sets bench (full size)
    "bench": {"fp32": dict(max_err=4.92e-7, mean_abs=6.33e-8, bytes_differ=0.0, max_byte_diff=0),
              "f16x3": dict(max_err=1.49e-6, mean_abs=2.02e-7, bytes_differ=0.00004, max_byte_diff=1),
              "f16": dict(max_err=3.24e-3, mean_abs=4.87e-4, bytes_differ=0.0624, max_byte_diff=1)},
}


def _f16(t):
    return t.clamp(-65504.0, 65504.0).half().double()


class _Stats:
    def __init__(self):
        self.convs = []            # (Cin, Cout, max |x|, max |w|)
        self.lo_nonzero = 0
        self.lo_subnormal = 0

    def lo(self, v):
        lo = (v - _f16(v)).clamp(-65504.0, 65504.0).half()
        nz = lo != 0
        self.lo_nonzero += int(nz.sum())
        self.lo_subnormal += int((nz & (lo.abs() < 2.0 ** -14)).sum())


def rounded_conv2d(mode, stats=None):
    """F.conv2d with the operands of the fp16-routed 3x3 convolutions rounded per `mode` (inputs fp64; the rest passes through)."""
    conv = F.conv2d

    def f(x, w, b=None, *args, **kw):
        if w.dim() != 4 or w.shape[-1] != 3 or w.shape[1] == 1 or args or kw:
            return conv(x, w, b, *args, **kw)
        x32, w32 = x.float().double(), w.float().double()
        if stats is not None:
            stats.convs.append((w.shape[1], w.shape[0], float(x.abs().max()), float(w.abs().max())))
            stats.lo(x32); stats.lo(w32)
        if mode == "fp32":
            return conv(x32, w32, b)
        xh, wh = _f16(x32), _f16(w32)
        if mode == "f16":
            return conv(xh, wh, b)
        xl, wl = _f16(x32 - xh), _f16(w32 - wh)
        return conv(xh, wh, b) + conv(xl, wh) + conv(xh, wl)
    return f


@contextlib.contextmanager
def patched_oracle(mode, stats=None):
    """The oracle's F.conv2d replaced by rounded_conv2d(mode) (the oracle module's own `F` name only)."""
    class _FP:
        def __getattr__(self, n):
            return getattr(F, n)
    proxy = _FP()
    proxy.conv2d = rounded_conv2d(mode, stats)
    old = spade_ref.F
    spade_ref.F = proxy
    try:
        yield
    finally:
        spade_ref.F = old


def emulate(sd, cfg, seg, z, mode, stats=None):
    """fp64 generator image with the operand rounding of `mode` (None: plain fp64)."""
    sd64 = {k: v.detach().double() for k, v in sd.items()}
    with torch.no_grad():
        if mode is None:
            return spade_ref.generator(sd64, cfg, seg.double(), z.double())
        with patched_oracle(mode, stats):
            return spade_ref.generator(sd64, cfg, seg.double(), z.double())


def to_bytes(img):
    return (((img.float() + 1.0) / 2.0).permute(0, 2, 3, 1) * 255.0).to(torch.uint8)      # save_color's conversion


def figures(img, truth):
    err = (img - truth).abs()
    bi, bt = to_bytes(img).int(), to_bytes(truth).int()
    return dict(max_err=float(err.max()) / float(truth.abs().max()), mean_abs=float(err.mean()),
                bytes_differ=float((bi != bt).double().mean()), max_byte_diff=int((bi - bt).abs().max()))


def weight_set(name, small):
    over = dict(ngf=8, nz=16, crop_size=64) if small else {}
    cfg = spade_ref.SpadeConfig(**over)
    if name == "oracle":
        sd = spade_ref.init_state(cfg, seed=7)
        seg, z = spade_ref.synth_input(cfg, 1, seed=3)
        return cfg, sd, seg, z
    from oracle.gen_golden_spade import BENCH_IMG_GAIN, BENCH_SEED        # bench.py's weights: torch's default init under its seed
    S = importlib.import_module("3d_sln_amd.host.SPADE_related")
    syn = importlib.import_module("3d_sln_amd.host.synthetic")
    torch.manual_seed(BENCH_SEED)
    G = S.SPADEGenerator4(cfg.semantic_nc, cfg.target_nc, cfg.nz, cfg.ngf, 'spectralspadelayer3x3', cfg.crop_size, 'normal')
    with torch.no_grad():
        G.conv_img.weight.mul_(BENCH_IMG_GAIN); G.conv_img.bias.mul_(BENCH_IMG_GAIN)
    seg, z = syn.spade_input(1, seed=BENCH_SEED)
    if small:
        seg = F.interpolate(seg, size=(cfg.crop_size, cfg.crop_size), mode="nearest")
        z = z[:, :cfg.nz]
    return cfg, {k: v.detach() for k, v in G.state_dict().items()}, seg, z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="ngf 8, 64 x 64 (seconds instead of minutes)")
    ap.add_argument("--sets", default="bench,oracle")
    a = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name in a.sets.split(","):
        cfg, sd, seg, z = weight_set(name, a.small)
        truth = emulate(sd, cfg, seg, z, None)
        print("== %s weights (%s)" % (name, "small" if a.small else "256 x 256, ngf 64"))
        print("%-6s %12s %10s %12s %10s" % ("mode", "max err/scl", "mean abs", "bytes != %", "max byte"))
        for mode in MODES:
            st = _Stats()
            f = figures(emulate(sd, cfg, seg, z, mode, st), truth)
            print("%-6s %12.2e %10.2e %12.3f %10d" % (mode, f["max_err"], f["mean_abs"], 100 * f["bytes_differ"], f["max_byte_diff"]))
        print("max |x| %.3g (conv %s), max |w| %.3g (conv %s); lo parts fp16-subnormal: %.2f %% of %d nonzero" % (
            max(c[2] for c in st.convs), max(st.convs, key=lambda c: c[2])[:2], max(c[3] for c in st.convs),
            max(st.convs, key=lambda c: c[3])[:2], 100.0 * st.lo_subnormal / max(st.lo_nonzero, 1), st.lo_nonzero))
        print("per conv (Cin, Cout, max |x|, max |w|):")
        for c in st.convs:
            print("  %4d %4d %8.3f %8.3f" % c)


if __name__ == "__main__":
    main()
