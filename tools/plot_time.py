"""Time the top-down layout pictures and the footprint heat map (host/plot2d.py) on the device, beside their torch restatements run on
the same device (the ATen baseline) and beside the centre-count launch of heatmap_from_words (sampling.layout_counts).

    python tools/plot_time.py
"""
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
P = importlib.import_module("3d_sln_amd.host.plot2d")
S = importlib.import_module("3d_sln_amd.host.sampling")
DEV = "cuda"


def layouts(n, n_obj, seed):
    """n layouts of n_obj object rows + the room row, in the decoder's output range"""
    g = torch.Generator().manual_seed(seed)
    size = 0.1 + 0.3 * torch.rand(n, n_obj, 3, generator=g)
    lo = torch.rand(n, n_obj, 3, generator=g) * (1.0 - size)
    room = torch.tensor([0, 0, 0, 1, 1, 1.0]).expand(n, 1, 6)
    boxes = torch.cat([torch.cat([lo, lo + size], -1), room], 1)
    bins = torch.cat([torch.randint(0, 24, (n, n_obj), generator=g), torch.zeros(n, 1, dtype=torch.int64)], 1)
    names = ["bed", "desk", "cabinet", "chair", "lamp", "sofa", "table", "television", "night_stand", "shelves"]
    objs = torch.tensor([P.PLOT2D_CLASSES.index(names[i % len(names)]) for i in range(n_obj)] + [0])
    rank, rgb = P.plot_tables(objs, P.PLOT2D_CLASSES)
    rr = torch.full((n_obj + 1,), n_obj, dtype=torch.int32)
    return [t.to(DEV) for t in (boxes, bins.float(), rr, rank, rgb)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    n, size = 4096, 256
    boxes, bins, rr, rank, rgb = layouts(n, 9, 1)
    ms = timed(lambda: P.layout_plot(boxes, bins, rr, rank, rgb, size=size), 10)
    print("layout_plot        S %5d x 1 room x %d^2, 10 rows: %8.3f ms  (%.0f layouts/s)" % (n, size, ms, n / ms * 1e3))
    sub = 256                                           # (the restatement holds [S, size, size] temporaries: a slice, scaled)
    ms_t = timed(lambda: P.layout_plot_torch(boxes[:sub], bins[:sub], rr, rank, rgb, size=size, dtype=torch.float32), 2) * n / sub
    print("layout_plot_torch  the same on the device (ATen, %d layouts x %d):   %8.3f ms  (%.0f layouts/s)" % (sub, n // sub, ms_t, n / ms_t * 1e3))

    n, size = 20000, 100
    boxes, bins, rr, rank, rgb = layouts(n, 9, 2)
    counts = torch.zeros(10, size, size, dtype=torch.int32, device=DEV)
    ms = timed(lambda: P.layout_footprints(boxes, bins, rr, rank, size=size, counts=counts), 10)
    print("layout_footprints  S %5d, O 10, N %d: %8.3f ms" % (n, size, ms))
    sub = 2000
    ms_t = timed(lambda: P.layout_footprints_torch(boxes[:sub], bins[:sub], rr, rank, size=size, dtype=torch.float32), 2) * n / sub
    print("layout_footprints_torch on the device (ATen, %d layouts x %d): %8.3f ms" % (sub, n // sub, ms_t))
    centres = torch.zeros(9, size, size, dtype=torch.float32, device=DEV)
    ms_c = timed(lambda: S.layout_counts(boxes, size, True, out=centres), 10)
    print("layout_counts      the centre-count launch of heatmap_from_words, the same layouts: %8.3f ms" % ms_c)


if __name__ == "__main__":
    main()
