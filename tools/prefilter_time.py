"""Timing of the reprojection of observed frames with and without the pre-filter (GPU box): tools/reproject_time.py's synthetic
640 x 480 frame into 256 x 256 refinement views, for 1 frame, for 16, and for ``ObservedFuser`` at 16 rooms x 4 views, in ONE process.

    python tools/prefilter_time.py [repeats] [--only 1,16,fuse]

Settings: ``prefilter`` = 1 (the unfiltered call: no filter is run), 2, 4 and ``prefilter_factor``'s choice for the frame and the view.
Settings and steps are interleaved so that a drift of the machine lands on all of them; per setting the median (p50) and the spread over
`repeats` windows of ITERS calls each (device events around a window), after two warm-up calls of everything:

  whole call                   ObservedReprojector / ObservedFuser: (filter,) faces, raster, compose or fuse
  sln_observed_prefilter       the filter alone (with its zero-fill of counts)
  sln_reproject_faces          the face step alone, on the frames the filter left
  sln_raster_forward           the rasterizer alone, on the faces the call left
  compose / fuse               the last step alone, on the maps the call left

and, per setting, the face slots per frame, the hits (pixels with a depth) and the filter's counts.  The last line per shape says whether
every window of the whole call at ``prefilter_factor``'s choice lies below every window of the unfiltered call.
"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
L = importlib.import_module("3d_sln_amd._lib")
RP = importlib.import_module("3d_sln_amd.host.reproject")
# the same frame, cameras, windows and steps of the route
from reproject_time import HS, WS, S, ITERS, ROOM, frame, window, pose_of, view_poses, steps, compose_step, fuse_step   # noqa: E402


def _run(title, settings, repeats, auto):
    """settings: [(f, object, variants)]"""
    for _, _, variants in settings:
        for _, fn in variants:
            for _ in range(2):
                fn()
    torch.cuda.synchronize()
    print("%s; %d windows of %d calls; per CALL: p50 [min .. max]" % (title, repeats, ITERS), flush=True)
    times = {(f, name): [] for f, _, variants in settings for name, _ in variants}
    for _ in range(repeats):
        for f, _, variants in settings:
            for name, fn in variants:
                times[(f, name)].append(window(fn))
    for f, o, variants in settings:
        variants[0][1]()
        torch.cuda.synchronize()
        counts = "" if o.pre is None else "; filter counts full / mixed / none (frame 0) %s" % o.pre.counts[0].tolist()
        print(" prefilter = %d%s: frames of %d x %d, %d face slots per frame, hits %d (%.1f %% of the pixels)%s" % (
            f, " (prefilter_factor's choice)" if f == auto else "", o.Wd, o.Hd, o.F, int(o.hits.sum()), 100.0 * int(o.hits.sum()) / o.depth.numel(), counts),
              flush=True)
        for name, _ in variants:
            t = sorted(times[(f, name)])
            print("   %-24s %10.1f us  [%9.1f .. %9.1f]" % (name, t[len(t) // 2] * 1e6, t[0] * 1e6, t[-1] * 1e6), flush=True)
    base, best = times[(1, "whole call")], times[(auto, "whole call")]
    if auto == 1:
        print(" prefilter_factor chooses 1 for this frame: nothing to compare", flush=True)
    else:
        print(" every window of the whole call at prefilter = %d below every window of the unfiltered call: %s (%.1f us max against %.1f us min; p50 x %.1f)" % (
            auto, max(best) < min(base), max(best) * 1e6, min(base) * 1e6, sorted(base)[len(base) // 2] / sorted(best)[len(best) // 2]), flush=True)


def measure(B, repeats):
    depth, labels, k_src = (t.cuda() for t in frame(B))
    K, _, _, orig = RP.refine_view(ROOM, S)
    auto = RP.prefilter_factor(k_src, K, orig, S)
    pose, K = pose_of(B), K[None].repeat(B, 1, 1).cuda()
    settings = []
    for f in sorted({1, 2, 4, auto}):
        rp = RP.ObservedReprojector(HS, WS, S, batch=B, prefilter=f)
        whole = (lambda rp: lambda: rp(depth, labels, k_src, pose, K, orig))(rp)
        settings.append((f, rp, steps(rp, "whole call", whole, depth, labels, k_src, pose, K, orig, "sln_reproject_compose", compose_step)))
    _run("ObservedReprojector: %d frame(s) of %d x %d into %d x %d" % (B, WS, HS, S, S), settings, repeats, auto)


def measure_fuser(R, V, repeats):
    B = R * V
    depth, labels, k_src = (t.cuda() for t in frame(B))
    K, _, _, orig = RP.refine_view(ROOM, S)
    auto = RP.prefilter_factor(k_src, K, orig, S)
    pose = view_poses(R, V)
    K = K[None].repeat(R, 1, 1).cuda()
    d4, l4, k4 = depth.view(R, V, HS, WS), labels.view(R, V, HS, WS), k_src.view(R, V, 4)
    settings = []
    for f in sorted({1, 2, 4, auto}):
        fu = RP.ObservedFuser(HS, WS, S, rooms=R, views=V, prefilter=f)
        whole = (lambda fu: lambda: fu(d4, l4, k4, pose, K, orig))(fu)
        whole()                                                      # (spreads K_tgt over the frames: the face step alone reads K_frames)
        settings.append((f, fu, steps(fu, "whole call", whole, depth, labels, k_src, pose.view(B, 3, 4), fu.K_frames, orig, "sln_reproject_fuse", fuse_step)))
    _run("ObservedFuser: %d rooms x %d views of %d x %d into %d x %d" % (R, V, WS, HS, S, S), settings, repeats, auto)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("repeats", nargs="?", type=int, default=7)
    ap.add_argument("--only", default="1,16,fuse", help="comma-separated: 1, 16 (frames of ObservedReprojector), fuse (16 rooms x 4 views)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefilter_time.py measures on the GPU; none found")
    for what in a.only.split(","):
        if what == "fuse":
            measure_fuser(16, 4, a.repeats)
        else:
            measure(int(what), a.repeats)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
