"""Timing of the reprojection of observed frames (GPU box): 640 x 480 frames into 256 x 256 refinement views, for 1 frame and for 16, in
ONE process.

    python tools/reproject_time.py [repeats]
    python tools/reproject_time.py [repeats] --views 1,2,4 [--rooms 16] [--frames 160x120,640x480]

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

With ``--views`` the fusion of V frames per room is measured instead (``ObservedFuser``; csrc/observed_fuse.hip): per frame size and V,
R rooms of V frames each, view v turned by a few degrees of its own so that the frames overlap in part:

  ObservedFuser                the whole call: K_tgt spread, faces and raster over R * V frames, the fused compose
  sln_reproject_fuse           the fused compose alone, on the maps the call left
  sln_reproject_compose        the parent's step on the same maps, as R * V separate frames: what V separate composes cost
  ObservedReprojector          (V = 1 only) the one-frame route on the same frames, in the same windows
"""
import argparse
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


def frame(B, seed=0, HS=HS, WS=WS):
    """-> depth_src [B, HS, WS], labels_src, k_src [B, 4] on the host (the picture of the 640 x 480 frame at any size)"""
    rng = np.random.default_rng(seed)
    q = WS / 640.0
    k = np.array([500.0 * q, 500.0 * q, WS / 2 + 0.3, HS / 2 - 0.2])
    rx, ry = (np.arange(WS) + 0.5 - k[2]) / k[0], (np.arange(HS) + 0.5 - k[3]) / k[1]
    out_d, out_l = [], []
    for b in range(B):
        wall = 4.0 + 0.2 * b / max(B - 1, 1)
        floor = 1.4 / np.maximum(ry, 1e-6)[:, None] + 0.0 * rx[None, :]            # the plane y = 1.4 (y runs down)
        d = np.minimum(np.full((HS, WS), wall), floor)
        lab = np.where(floor < wall, 2, 1).astype(np.uint8)                       # floor / wall
        i0, j0 = int(q * (300 + int(rng.integers(0, 40)))), int(q * (200 + int(rng.integers(0, 200))))
        d[i0:i0 + int(90 * q), j0:j0 + int(140 * q)] *= 0.7; lab[i0:i0 + int(90 * q), j0:j0 + int(140 * q)] = 4     # a box nearer than what is behind it
        d[:, int(10 * q):int(10 * q) + max(1, int(4 * q))] = np.nan               # a band without a reading
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


ROOM = [0.0, 0.0, 0.0, 4.0, 2.7, 5.0]


def pose_of(B):
    """[B, 3, 4] on the device: the small rotation and translation of the one-frame route"""
    c, s = np.cos(0.05), np.sin(0.05)
    return torch.tensor([[c, 0.0, s, 0.1], [0.0, 1.0, 0.0, -0.05], [-s, 0.0, c, 0.2]], dtype=torch.float32)[None].repeat(B, 1, 1).cuda()


def view_poses(R, V):
    """[R, V, 3, 4] on the device: view v looks a few degrees to the side of the others"""
    poses = []
    for v in range(V):
        a = 0.05 + 0.06 * (v - 0.5 * (V - 1))
        c, s = np.cos(a), np.sin(a)
        poses.append([[c, 0.0, s, 0.1 - 0.15 * (v - 0.5 * (V - 1))], [0.0, 1.0, 0.0, -0.05], [-s, 0.0, c, 0.2]])
    return torch.tensor(poses, dtype=torch.float32)[None].repeat(R, 1, 1, 1).contiguous().cuda()


def compose_step(o, lab):
    RP.compose(o.face_index, o.weight, o.raster_depth, lab, o.depth, o.labels, o.hits)


def fuse_step(o, lab):
    RP.fuse(o.face_index, o.weight, o.raster_depth, lab, o.views, o.gap, o.depth, o.labels, o.hits, o.source, o.count, o.agree, o.wins)


def steps(o, whole_name, whole, dep, lab, k, pose, K, orig, last_name, last):
    """the variants of one route object: the whole call and its steps on what the call left; dep, lab, k, pose, K are the flat frames
    as the face step takes them without a filter (prefilter_time.py times the same steps per setting)"""
    v = [(whole_name, whole)]
    if o.pre is not None:
        v.append(("sln_observed_prefilter", lambda src=(dep, lab, k): o.pre(*src)))
        dep, lab, k = o.pre.depth, o.pre.labels, o.pre.k_out
    v.append(("sln_reproject_faces", lambda: RP.faces(dep, k, pose, K, orig, o.near, o.gap, o.faces_xyz)))
    v.append(("sln_raster_forward", o.raster))
    v.append((last_name, lambda: last(o, lab)))
    return v


def measure(B, repeats):
    depth, labels, k_src = (t.cuda() for t in frame(B))
    K, R, t, orig = RP.refine_view(ROOM, S)
    pose = pose_of(B)
    K = K[None].repeat(B, 1, 1).cuda()
    rp = RP.ObservedReprojector(HS, WS, S, batch=B)
    variants = steps(rp, "ObservedReprojector", lambda: rp(depth, labels, k_src, pose, K, orig), depth, labels, k_src, pose, K, orig,
                     "sln_reproject_compose", compose_step)
    variants += [("torch: faces", lambda: RP.faces_torch(depth, k_src, pose, K, orig, rp.near, rp.gap, torch.float32)),
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
    report(variants, times)
    d_t, l_t, h_t = RP.compose_torch(rp.face_index, rp.weight, rp.raster_depth, labels)
    print("   [check] the compose kernel equals the torch compose on the device's maps: %s"
          % bool(torch.equal(d_t.view(torch.int32), rp.depth.view(torch.int32)) and torch.equal(l_t, rp.labels) and torch.equal(h_t, rp.hits)), flush=True)


def report(variants, times):
    for name, _ in variants:
        v = sorted(times[name])
        print("   %-24s %10.1f us  [%9.1f .. %9.1f]" % (name, v[len(v) // 2] * 1e6, v[0] * 1e6, v[-1] * 1e6), flush=True)


def measure_views(R, V, Hs, Ws, repeats):
    B = R * V
    depth, labels, k_src = (t.cuda() for t in frame(B, HS=Hs, WS=Ws))
    K, _, _, orig = RP.refine_view(ROOM, S)
    pose = view_poses(R, V)
    K = K[None].repeat(R, 1, 1).cuda()
    depth, labels, k_src = depth.view(R, V, Hs, Ws), labels.view(R, V, Hs, Ws), k_src.view(R, V, 4)
    fu = RP.ObservedFuser(Hs, Ws, S, rooms=R, views=V)
    flat_labels = labels.view(B, Hs, Ws)
    c_depth, c_labels = torch.empty(B, S, S, device="cuda"), torch.empty(B, S, S, dtype=torch.uint8, device="cuda")
    c_hits = torch.zeros(B, dtype=torch.int64, device="cuda")
    variants = [("ObservedFuser", lambda: fu(depth, labels, k_src, pose, K, orig)),
                ("sln_reproject_fuse", lambda: fuse_step(fu, flat_labels)),
                ("sln_reproject_compose", lambda: RP.compose(fu.face_index, fu.weight, fu.raster_depth, flat_labels, c_depth, c_labels, c_hits))]
    if V == 1:
        rp = RP.ObservedReprojector(Hs, Ws, S, batch=R)
        one = (depth.view(B, Hs, Ws), flat_labels, k_src.view(B, 4), pose.view(B, 3, 4), K, orig)
        variants.append(("ObservedReprojector", lambda: rp(*one)))
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    n = float(R * S * S)
    print("%d room(s) x %d view(s) of %d x %d into %d x %d, %d face slots per frame; winners %.1f %% of the pixels, seen by two or more %.1f %%, wins per view "
          "(room 0) %s; %d windows of %d calls; per CALL: p50 [min .. max]"
          % (R, V, Ws, Hs, S, S, fu.F, 100.0 * int(fu.hits.sum()) / n, 100.0 * int((fu.count >= 2).sum()) / n, fu.wins[0].tolist(), repeats, ITERS), flush=True)
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window(fn))
    report(variants, times)
    want = RP.fuse_torch(fu.face_index, fu.weight, fu.raster_depth, flat_labels, V, fu.gap)
    same = all(torch.equal(want[k], getattr(fu, k)) for k in ("labels", "source", "count", "agree", "hits", "wins"))
    print("   [check] the fuse kernel equals fuse_torch on the device's maps: %s"
          % bool(same and torch.equal(want["depth"].view(torch.int32), fu.depth.view(torch.int32))), flush=True)
    if V == 1:
        print("   [check] ObservedFuser(views=1) equals ObservedReprojector: %s"
              % bool(torch.equal(rp.depth.view(torch.int32), fu.depth.view(torch.int32)) and torch.equal(rp.labels, fu.labels) and torch.equal(rp.hits, fu.hits)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--views", default=None, help="comma-separated V: measure the fusion of V frames per room instead")
    ap.add_argument("--rooms", type=int, default=16)
    ap.add_argument("--frames", default="160x120,640x480", help="comma-separated WxH of the source frames (with --views)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reproject_time.py measures on the GPU; none found")
    if a.views is None:
        for B in (1, 16):
            measure(B, a.repeats)
        return
    for size in a.frames.split(","):
        Ws, Hs = (int(x) for x in size.lower().split("x"))
        for V in (int(x) for x in a.views.split(",")):
            measure_views(a.rooms, V, Hs, Ws, a.repeats)


if __name__ == "__main__":
    main()
