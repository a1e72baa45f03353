"""Time the posterior heat-map application (reference testing/test_heatmap.py: 20 000 single-graph decodes) on the GPU box.

    python tools/heatmap_time.py [--precision fp32,f16x3,f16] [--samples 20000,4096,256] [--windows 9] [--reps 20]

Per sample count, the precision modes (Sg2ScVAEModel.gemm_precision) alternate in ONE process: `windows` timed windows per mode,
each `reps` whole heat maps (z draw, decode of all samples in one engine call, histogram launch) between two device synchronisations.
Printed per mode: the median (p50), fastest and slowest window in ms per heat map, the spread (slowest - fastest), layouts/s at the
median, and the largest difference of the normalised heat map from the fp32 one on the same z (a CPU generator with one seed)."""
import argparse
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32", help="comma-separated: fp32, f16x3, f16")
    ap.add_argument("--samples", default="20000", help="comma-separated sample counts (layouts per heat map)")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20, help="heat maps per timed window")
    a = ap.parse_args()
    modes = a.precision.split(",")
    M = importlib.import_module("3d_sln_amd.host.Sg2ScVAE_model")
    syn = importlib.import_module("3d_sln_amd.host.synthetic")
    S = importlib.import_module("3d_sln_amd.host.sampling")
    torch.manual_seed(0)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64,
                            gconv_mode='feedforward', gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32,
                            use_AE=False).cuda().eval()
    objs5 = ["bed", "desk", "cabinet", "chair", "lamp"]
    rels5 = [("bed", "behind", "desk"), ("cabinet", "left of", "bed"), ("chair", "left of", "desk"), ("lamp", "on", "desk")]
    mean = torch.zeros(64, dtype=torch.float64); cov = torch.eye(64, dtype=torch.float64)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for n in [int(v) for v in a.samples.split(",")]:
            maps = {}
            for m in modes:                                   # warm-up of every (shape, mode) and the same-z comparison
                S.heatmap_from_words(model, objs5, rels5, mean, cov, num_iter=n, chunk=n, precision=m)
                maps[m] = S.heatmap_from_words(model, objs5, rels5, mean, cov, num_iter=n, chunk=n, precision=m,
                                               generator=torch.Generator().manual_seed(1)).cpu()
            torch.cuda.synchronize()
            times = {m: [] for m in modes}
            for _ in range(a.windows):
                for m in modes:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        S.heatmap_from_words(model, objs5, rels5, mean, cov, num_iter=n, chunk=n, precision=m)
                    torch.cuda.synchronize()
                    times[m].append((time.perf_counter() - t0) / a.reps * 1e3)
            for m in modes:
                t = sorted(times[m])
                p50 = t[len(t) // 2]
                diff = float((maps[m] - maps[modes[0]]).abs().max())
                print("%6d layouts %-6s p50 %8.3f ms  min %8.3f  max %8.3f  spread %7.3f  %10.0f layouts/s  max |heat map - %s| %.2e" % (
                    n, m, p50, t[0], t[-1], t[-1] - t[0], n / p50 * 1e3, modes[0], diff))


if __name__ == "__main__":
    main()
