"""Timing of the reprojection of observed frames (GPU box): 640 x 480 frames into 256 x 256 refinement views, for 1 frame and for 16, in
ONE process.

    python tools/reproject_time.py [repeats]

The frame is synthetic: a floor and a back wall seen by a 500-pixel lens from 1.4 m up, with a box on the floor (depth steps on its rim),
a band of pixels without a reading and class bytes in blocks.  The target is ``refine_view`` of a 4 x 2.7 x 5 room, the pose a small
rotation and translation.  Variants are interleaved so that a drift of the machine lands on all of them; per variant the median (p50) and
the spread over `repeats` windows of ITERS calls each (device events around a window), after two warm-up calls of every variant:

  ObservedReprojector          the whole call: faces, raster, compose
  sln_reproject_faces          step 1 alone
  sln_raster_forward           step 2 alone, on the faces step 1 left
  sln_reproject_compose        step 3 alone, on the maps step 2 left
  torch: faces                 ``faces_torch`` in float32 on the device (what step 1 replaces)
  torch: compose               ``compose_torch`` on the device (what step 3 replaces)
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = importlib.import_module("3d_sln_amd._lib")
RP = importlib.import_module("3d_sln_amd.host.reproject")

ITERS = int(os.environ.get("ITERS", "10"))
HS, WS, S = 480, 640, 256


def frame(B, seed=0):
    """-> depth_src [B, HS, WS], labels_src, k_src [B, 4] on the host"""
    rng = np.random.default_rng(seed)
    k = np.array([500.0, 500.0, WS / 2 + 0.3, HS / 2 - 0.2])
    rx, ry = (np.arange(WS) + 0.5 - k[2]) / k[0], (np.arange(HS) + 0.5 - k[3]) / k[1]
    out_d, out_l = [], []
    for b in range(B):
        wall = 4.0 + 0.2 * b / max(B - 1, 1)
        floor = 1.4 / np.maximum(ry, 1e-6)[:, None] + 0.0 * rx[None, :]            # the plane y = 1.4 (y runs down)
        d = np.minimum(np.full((HS, WS), wall), floor)
        lab = np.where(floor < wall, 2, 1).astype(np.uint8)                       # floor / wall
        i0, j0 = 300 + int(rng.integers(0, 40)), 200 + int(rng.integers(0, 200))
        d[i0:i0 + 90, j0:j0 + 140] *= 0.7; lab[i0:i0 + 90, j0:j0 + 140] = 4        # a box nearer than what is behind it
        d[:, 10:14] = np.nan                                                      # a band without a reading
        out_d.append(d.astype(np.float32)); out_l.append(lab)
    return torch.from_numpy(np.stack(out_d)), torch.from_numpy(np.stack(out_l)), torch.from_numpy(np.tile(k, (B, 1)).astype(np.float32))


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e-3


def measure(B, repeats):
    depth, labels, k_src = (t.cuda() for t in frame(B))
    K, R, t, orig = RP.refine_view([0.0, 0.0, 0.0, 4.0, 2.7, 5.0], S)
    c, s = np.cos(0.05), np.sin(0.05)
    pose = torch.tensor([[c, 0.0, s, 0.1], [0.0, 1.0, 0.0, -0.05], [-s, 0.0, c, 0.2]], dtype=torch.float32)[None].repeat(B, 1, 1).cuda()
    K = K[None].repeat(B, 1, 1).cuda()
    rp = RP.ObservedReprojector(HS, WS, S, batch=B)
    lib, P, st = L.lib(), L.ptr, L.current_stream_ptr

    def raster():
        L.check(lib.sln_raster_forward(P(rp.faces_xyz), B, rp.F, S, rp.near, rp.far, P(rp._raster_ws), P(rp.face_index), P(rp.weight), P(rp.raster_depth),
                                       st()), "sln_raster_forward")
    variants = [("ObservedReprojector", lambda: rp(depth, labels, k_src, pose, K, orig)),
                ("sln_reproject_faces", lambda: RP.faces(depth, k_src, pose, K, orig, rp.near, rp.gap, rp.faces_xyz)),
                ("sln_raster_forward", raster),
                ("sln_reproject_compose", lambda: RP.compose(rp.face_index, rp.weight, rp.raster_depth, labels, rp.depth, rp.labels, rp.hits)),
                ("torch: faces", lambda: RP.faces_torch(depth, k_src, pose, K, orig, rp.near, rp.gap, torch.float32)),
                ("torch: compose", lambda: RP.compose_torch(rp.face_index, rp.weight, rp.raster_depth, labels))]
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    kept = int((~(rp.faces_xyz == 0).all(-1).all(-1)).sum())
    print("%d frame(s) of %d x %d into %d x %d, %d face slots per frame (%.1f %% kept), hits per frame %s; %d windows of %d calls; per CALL: p50 [min .. max]"
          % (B, WS, HS, S, S, rp.F, 100.0 * kept / (B * rp.F), rp.hits.tolist(), repeats, ITERS), flush=True)
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window(fn))
    for name, _ in variants:
        v = sorted(times[name])
        print("   %-24s %10.1f us  [%9.1f .. %9.1f]" % (name, v[len(v) // 2] * 1e6, v[0] * 1e6, v[-1] * 1e6), flush=True)
    d_t, l_t, h_t = RP.compose_torch(rp.face_index, rp.weight, rp.raster_depth, labels)
    print("   [check] the compose kernel equals the torch compose on the device's maps: %s"
          % bool(torch.equal(d_t.view(torch.int32), rp.depth.view(torch.int32)) and torch.equal(l_t, rp.labels) and torch.equal(h_t, rp.hits)), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("reproject_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    for B in (1, 16):
        measure(B, repeats)


if __name__ == "__main__":
    main()
