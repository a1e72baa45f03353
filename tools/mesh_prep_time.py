"""Timing of the edge splitter (GPU box): ``mesh_prep.split_meshes`` / ``split_long_edges`` on device tensors (csrc/mesh_split.hip: three
launches per pass, torch's unique / cumsum and one read-back between them) beside ``split_long_edges_np`` on the host, max_edge 0.6:

    bank        32 classes x 8 cuboid models (12 triangles each, edges 0.25 .. 2.5) in ONE split_meshes call
    room box    the 12 x 3 x 9 cuboid: 12 -> 6 144 faces in 5 passes
    one by one  the same bank, one split_long_edges call per mesh

    python tools/mesh_prep_time.py [repeats]

Wall-clock per call with a device synchronisation at its end (the call reads back once per pass, so device events alone would miss
the host's share), the median and the spread over `repeats` calls after one warm-up, the variants alternated; before timing, the device
result is asserted equal to the host's on every mesh.  The inputs are on their device before the clock starts.  There is no bar: the
figures go to LAB_NOTES.
"""
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MP = importlib.import_module("3d_sln_amd.host.mesh_prep")

MAX_EDGE = 0.6
N_CLASSES, PER_CLASS = 32, 8


def cuboid(size):
    sx, sy, sz = size
    v = np.array([[x, y, z] for x in (0.0, sx) for y in (0.0, sy) for z in (0.0, sz)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)


def bank(rng):
    return [cuboid(rng.integers(1, 11, size=3) / 4.0) for _ in range(N_CLASSES * PER_CLASS)]


def timed(fn, sync):
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def same(dev, host):
    return dev[0].cpu().numpy().tobytes() == host[0].tobytes() and np.array_equal(dev[1].cpu().numpy(), host[1])


def main():
    if not torch.cuda.is_available():
        raise SystemExit("mesh_prep_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    meshes = bank(np.random.default_rng(0))
    dmeshes = [(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()) for v, f in meshes]
    room = cuboid((12.0, 3.0, 9.0))
    droom = tuple(torch.from_numpy(x).cuda() for x in room)
    work = {
        "bank, one call": (lambda: MP.split_meshes(dmeshes, MAX_EDGE), lambda: MP.split_meshes(meshes, MAX_EDGE)),
        "room box": (lambda: [MP.split_long_edges(*droom, MAX_EDGE)], lambda: [MP.split_long_edges_np(*room, MAX_EDGE)]),
        "bank, one by one": (lambda: [MP.split_long_edges(v, f, MAX_EDGE) for v, f in dmeshes],
                             lambda: [MP.split_long_edges_np(v, f, MAX_EDGE) for v, f in meshes]),
    }
    for name, (dev, host) in work.items():
        d, h = timed(dev, True)[1], timed(host, False)[1]                  # warm-up, and the check
        assert len(d) == len(h) and all(same(a, b) for a, b in zip(d, h)), name
        faces_in, faces_out = sum(int(m[2]["origin"].max()) + 1 for m in h), sum(int(m[1].shape[0]) for m in h)
        times = {"device": [], "numpy": []}
        for _ in range(repeats):
            times["device"].append(timed(dev, True)[0])
            times["numpy"].append(timed(host, False)[0])
        for k, t in times.items():
            t = np.sort(np.asarray(t))
            print("%-17s %6d -> %7d faces, passes <= %d  %-6s p50 %9.2f ms  (min %.2f, max %.2f; %d calls)" % (
                name, faces_in, faces_out, max(m[2]["passes"] for m in h), k, 1e3 * np.median(t), 1e3 * t[0], 1e3 * t[-1], repeats))


if __name__ == "__main__":
    main()
