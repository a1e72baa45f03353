"""Timing of the SPADE input builder (GPU box): the ATen path ``build_input`` beside ``InputBuilder`` with uint8 masks and with a
class-index image, in ONE process, on the 1024 x 1024 golden scene (depth + 4 masks: 5 live channels) and on a scene in which all
41 channels are live.

    python tools/spade_input_time.py [repeats]

Per variant: the median (p50) and the spread over `repeats` windows of ITERS calls each (device events around a window, the variants
interleaved so that a drift of the machine lands on all of them), the bytes the work has to move by its definition - the depth once,
one byte per pixel of every mask (or the one label image), the [41, 256, 256] float32 result once - and that over the time as a
fraction of the HBM peak (8.0 TB/s datasheet; a float4 copy reaches 6.29).  What the kernels actually move is more: the depth is
read three times (minimum, maximum, resize), and a row tile's band overlaps its neighbours' (L2 hits at these sizes).
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S = importlib.import_module("3d_sln_amd.host.spade_input")
from oracle import spade_input_ref as R          # noqa: E402  (the golden scene's generator; test infrastructure, not product code)

HBM_PEAK = 8.0e12
ITERS = int(os.environ.get("ITERS", "20"))


def scenes():
    depth, masks = R.synth_scene(1024, seed=2)
    names = list(masks)
    planes = torch.from_numpy(np.stack([masks[k] for k in names])).to(torch.uint8).cuda()
    labels = torch.zeros(1024, 1024, dtype=torch.uint8, device="cuda")
    for j, k in enumerate(names):                                                # overlapping masks: the later class wins (timing only)
        labels[planes[j] > 120] = 1 + S.NYU40.index(k)
    yield "golden scene, 5 live channels", torch.from_numpy(depth).cuda(), planes, names, labels
    rng = np.random.default_rng(0)
    lab = torch.from_numpy(rng.integers(1, 41, size=(128, 128)).astype(np.uint8)).cuda().repeat_interleave(8, 0).repeat_interleave(8, 1)
    planes = torch.stack([(lab == 1 + c).to(torch.uint8) * 255 for c in range(40)])
    yield "all 41 channels live", torch.from_numpy(depth).cuda(), planes, list(S.NYU40), lab


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e-3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("spade_input_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out_bytes = 41 * 256 * 256 * 4
    print("SPADE input builder, 1024 x 1024 -> [1, 41, 256, 256]; %d windows of %d calls, device events; p50 [min .. max]" % (repeats, ITERS))
    for title, depth, planes, names, labels in scenes():
        builder = S.InputBuilder(1024, 1024, size=256)
        as_dict = {k: planes[j] for j, k in enumerate(names)}
        chan = builder._channel_table(names, len(names))
        variants = [
            ("build_input (ATen, parent path)", lambda: S.build_input(depth, as_dict, size=256), None),
            ("InputBuilder, uint8 masks", lambda: builder(depth, masks=planes, channels=chan), depth.numel() * 4 + planes.numel() + out_bytes),
            ("InputBuilder, label image", lambda: builder(depth, labels=labels), depth.numel() * 4 + labels.numel() + out_bytes),
        ]
        # the label image holds one class per pixel and no greys: its yardstick is build_input on the masks it expands to
        wants = (variants[0][1](), S.build_input(depth, S.masks_from_labels(labels), size=256))
        for (name, fn, _), want in zip(variants[1:], wants):
            err = ((fn() - want).abs() / want.abs().clamp(min=1)).max().item()
            print("   [check] %-32s largest error against build_input / max(1, |want|): %.2e" % (name, err))
        del wants
        for _, fn, _ in variants:                                                # warm-up: code objects, allocator, BLAS choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in variants}
        for _ in range(repeats):
            for name, fn, _ in variants:
                times[name].append(window(fn))
        print(title)
        base = None
        for name, _, nbytes in variants:
            v = sorted(times[name])
            p50 = v[len(v) // 2]
            base = base or p50
            line = "   %-32s %9.1f us  [%8.1f .. %8.1f]   x%6.1f" % (name, p50 * 1e6, v[0] * 1e6, v[-1] * 1e6, base / p50)
            if nbytes:
                line += "   %5.1f MB to move, %6.3f TB/s = %4.1f %% of the HBM peak" % (nbytes / 1e6, nbytes / p50 / 1e12, 100 * nbytes / p50 / HBM_PEAK)
            print(line, flush=True)


if __name__ == "__main__":
    main()
