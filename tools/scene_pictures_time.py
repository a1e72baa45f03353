"""Timing of the refinement pictures (GPU box): ``scene_pictures_torch`` (the ATen restatement, on the same device tensors) beside
``ScenePictures`` in ONE process, on 16 rooms x 70 x 256 x 256 with 5 live semantic classes a room (the planes of the other classes
flagged dead, as the sparse scene pass leaves them) and with all planes live, with and without ``masks8``.

    python tools/scene_pictures_time.py [repeats]

Per variant: the median (p50) and the spread over `repeats` windows of ITERS calls each (device events around a window, the variants
alternated so that a drift of the machine lands on all of them), and the bytes the work has to move by its definition: the depth plane
three times (minimum, maximum, pixels), every live semantic plane once, one byte a pixel for depth8 and labels, three for rgb, forty for
masks8 - over the time as a fraction of the HBM peak (8.0 TB/s datasheet; a float4 copy reaches 6.29).  The comparison point is the
ATen restatement, not the kernel itself.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SP = importlib.import_module("3d_sln_amd.host.scene_pictures")

HBM_PEAK = 8.0e12
ITERS = int(os.environ.get("ITERS", "20"))
B, C, S = 16, 70, 256


def rooms(n_classes):
    """-> (image [B, C, S, S], live [B, C]): 8 x 8-pixel cells, `n_classes` classes a room, depth in [1, 8] over a -1 background"""
    rng = np.random.RandomState(n_classes)
    img = np.zeros((B, C, S, S), np.float32)
    live = np.full((B, C), 3, np.uint8)
    for b in range(B):
        classes = rng.choice(40, n_classes, replace=False)
        cell = rng.randint(-1, n_classes, size=(S // 8, S // 8)).repeat(8, 0).repeat(8, 1)                  # -1: background
        img[b, 0] = np.where(cell < 0, -1.0, rng.randint(64, 512, size=(S // 8, S // 8)).repeat(8, 0).repeat(8, 1) / 64.0)
        for j, c in enumerate(classes):
            img[b, 1 + c] = cell == j
        dead = np.setdiff1d(np.arange(40), classes)
        live[b, 1 + dead] = 0
        img[b, 41:] = 1.0
        live[b, 41:] = 1
    return torch.from_numpy(img).cuda(), torch.from_numpy(live).cuda()


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
        raise SystemExit("scene_pictures_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    n = S * S
    print("refinement pictures, %d rooms x %d x %d x %d; %d windows of %d calls, device events; p50 [min .. max]" % (B, C, S, S, repeats, ITERS))
    for n_classes in (5, 40):
        image, live = rooms(n_classes)
        flags = live if n_classes < 40 else None
        variants = []
        for masks in (False, True):
            sp = SP.ScenePictures(S, batch=B, channels=C, masks=masks)
            moved = B * n * (3 * 4 + n_classes * 4 + 1 + 1 + 3 + (40 if masks else 0))
            tag = "masks8" if masks else "no masks8"
            variants.append(("scene_pictures_torch (ATen), " + tag, lambda m=masks: SP.scene_pictures_torch(image, flags, masks=m), None, None))
            variants.append(("ScenePictures, " + tag, lambda s=sp: s(image, flags), moved, sp))
        for k in (0, 2):                                                         # the kernel against the restatement, every byte
            want, got = variants[k][1](), variants[k + 1][1]()
            diff = sum(int((a != b).sum()) for a, b in zip(want, got) if a is not None)
            print("   [check] %-28s differing bytes against the restatement: %d" % (variants[k + 1][0], diff))
        for _, fn, _, _ in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _, _ in variants}
        for _ in range(repeats):
            for name, fn, _, _ in variants:
                times[name].append(window(fn))
        print("%d live classes a room%s" % (n_classes, ", the others flagged dead" if flags is not None else ", live=None"))
        base = None
        for i, (name, _, nbytes, _) in enumerate(variants):
            v = sorted(times[name])
            p50 = v[len(v) // 2]
            if nbytes is None:
                base = p50
            line = "   %-42s %9.1f us  [%8.1f .. %8.1f]   x%6.1f" % (name, p50 * 1e6, v[0] * 1e6, v[-1] * 1e6, base / p50)
            if nbytes:
                line += "   %6.1f MB to move, %6.3f TB/s = %4.1f %% of the HBM peak" % (nbytes / 1e6, nbytes / p50 / 1e12, 100 * nbytes / p50 / HBM_PEAK)
            print(line, flush=True)


if __name__ == "__main__":
    main()
