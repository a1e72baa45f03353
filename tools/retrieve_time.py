"""Timing of the mesh retrieval (GPU box): ``retrieve_models`` (csrc/mesh_retrieve.hip) beside ``retrieve_models_torch`` (the ATen
restatement, on the same device tensors) in ONE process, against a table of 2 600 models in 40 classes (the size of the SUNCG table:
a few classes with hundreds of models, most with a few dozen):

    16 rooms x 12 rows        what one RefineBatch retrieves at set-up
    20 000 layouts x 12 rows  furnishing the samples of heatmap_from_words / sample_layouts (240 k rows)

    python tools/retrieve_time.py [repeats]

Per shape and variant: the median (p50) and the spread over `repeats` windows of ITERS calls each (device events around a window, the
variants alternated so that a drift of the machine lands on both), after asserting that both give the same choice on every row.
The restatement is a host loop over the classes with a [rows, models of the class] distance matrix per class; its time includes that
loop's launches.  There is no bar: the figures go to LAB_NOTES.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RT = importlib.import_module("3d_sln_amd.host.retrieve")

ITERS = int(os.environ.get("ITERS", "5"))
N_MODELS, N_CLASSES, ROWS = 2600, 40, 12


def table(rng):
    share = rng.dirichlet(np.full(N_CLASSES, 0.5))
    counts = np.maximum(1, np.floor(share * N_MODELS).astype(int))
    counts[np.argmax(counts)] += N_MODELS - counts.sum()
    vocab = ["__room__"] + ["c%02d" % c for c in range(N_CLASSES)]
    data = {}
    for name, n in zip(vocab[1:], counts):
        lo = rng.uniform(-1, 1, size=(n, 3))
        data[name] = [{"id": "%s_%d" % (name, k), "bbox_min": lo[k].tolist(), "bbox_max": (lo[k] + rng.uniform(0.3, 2.0, size=3)).tolist()}
                      for k in range(n)]
    return RT.ModelTable(data, vocab, "cuda"), counts


def layouts(rng, rooms):
    n = rooms * ROWS
    lo = rng.uniform(0.0, 0.6, size=(n, 3))
    boxes = np.concatenate([lo, lo + rng.uniform(0.05, 0.4, size=(n, 3))], 1).astype(np.float32)
    objs = rng.integers(1, N_CLASSES + 1, size=n).astype(np.int32)
    last = np.arange(rooms) * ROWS + ROWS - 1
    boxes[last] = np.concatenate([np.zeros((rooms, 3)), rng.uniform(2.5, 7.0, size=(rooms, 3))], 1)
    objs[last] = 0
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(objs).cuda(), torch.from_numpy(np.repeat(last, ROWS).astype(np.int32)).cuda()


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
        raise SystemExit("retrieve_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    rng = np.random.default_rng(0)
    tab, counts = table(rng)
    print("table: %d models in %d classes (largest %d, median %d)" % (tab.n_models, N_CLASSES, counts.max(), int(np.median(counts))))
    for rooms in (16, 20000):
        boxes, objs, room_row = layouts(rng, rooms)
        b3 = boxes[None].contiguous()
        choice = torch.empty(1, boxes.shape[0], dtype=torch.int32, device="cuda")
        fns = {"kernel": lambda: RT.into(b3, objs, room_row, tab, choice), "torch": lambda: RT.retrieve_models_torch(boxes, objs, room_row, tab)}
        fns["kernel"]()
        want = fns["torch"]()
        torch.cuda.synchronize()
        assert torch.equal(choice[0], want), "%d rows differ" % int((choice[0] != want).sum())
        times = {k: [] for k in fns}
        for _ in range(repeats):
            for k, fn in fns.items():
                times[k].append(window(fn))
        for k, t in times.items():
            t = np.sort(np.asarray(t))
            print("%6d rooms x %d rows  %-6s p50 %10.1f us  (min %.1f, max %.1f; %d windows of %d)" % (rooms, ROWS, k, 1e6 * np.median(t), 1e6 * t[0],
                                                                                                      1e6 * t[-1], repeats, ITERS))


if __name__ == "__main__":
    main()
