"""Timing of the viewpoint render (GPU box): ``ViewRenderer`` beside the ATen composition of the same steps, in ONE process, per room at
1024 x 1024 with 5 candidate views, and the share of ``sln_raster_forward`` in it.

    python tools/shade_time.py [repeats]

The room: 12 objects of a procedural bank (one cuboid model of 1728 faces per class) and the procedural shell.  Variants, interleaved so
that a drift of the machine lands on all of them; per variant the median (p50) and the spread over `repeats` windows of ITERS calls each
(device events around a window):

  ATen composition      ``row_tables`` + ``place_project_torch`` + ``sln_raster_forward`` + ``compose_torch`` + ``choose_view`` on the device:
                        the two new kernels replaced by the torch ops that restate them (there is no ATen rasterizer: both rows rasterise with
                        the same kernel)
  ViewRenderer          the whole call
  per-row tables        the vectorised fp32 torch ops in front of the first kernel (both rows share them)
  place + project       ``sln_view_place_project`` alone
  sln_raster_forward    alone, on the renderer's own faces: its share of the ViewRenderer row is printed
  compose               ``sln_view_compose`` alone (two launches)
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SH = importlib.import_module("3d_sln_amd.host.shade")
RF = importlib.import_module("3d_sln_amd.host.refine")
L = importlib.import_module("3d_sln_amd._lib")

ITERS = int(os.environ.get("ITERS", "10"))
SIZE, VIEWS = int(os.environ.get("SIZE", "1024")), 5


def room(bank, n=12, seed=0):
    rng = np.random.default_rng(seed)
    vocab = bank.table_vocab()
    names = [nm for nm in vocab[1:] if nm in bank.models]
    cls = np.array([vocab.index(nm) for nm in rng.choice(names, size=n, replace=False)] + [0])
    lo = rng.uniform([0.05, 0.0, 0.05], [0.7, 0.0, 0.6], size=(n, 3))
    boxes = np.concatenate([np.concatenate([lo, lo + rng.uniform(0.1, 0.3, size=(n, 3))], 1), [[0, 0, 0, 4.0, 2.7, 5.0]]]).astype(np.float32)
    angles = np.concatenate([rng.integers(0, 24, size=n), [0]]).astype(np.float32)
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(angles).cuda(), torch.from_numpy(cls).cuda(), [n + 1]


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
        raise SystemExit("shade_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    names = [n for n in importlib.import_module("3d_sln_amd.host.synthetic").FURNITURE if n in SH.NYU40]
    bank = RF.MeshBank(names, "cuda", subdiv=12)
    boxes, angles, objs, rows = room(bank)
    draws = torch.rand(1, VIEWS, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    r = SH.ViewRenderer(bank, size=SIZE, views=VIEWS, batch=1)
    r(boxes, angles, objs, rows, draws=draws)
    torch.cuda.synchronize()
    tables, bind = r.tables, r._bind
    print("viewpoint render, 1 room x %d views at %d x %d, %d face slots (%d rows x %d + %d shell); %d windows of %d calls; p50 [min .. max]"
          % (VIEWS, SIZE, SIZE, r.F, bind.N, tables.Fm, tables.Fs, repeats, ITERS))

    def prepare():
        rt = SH.row_tables(tables, bind, boxes, angles, objs, None, torch.float32)
        K, Rm, t = SH.shade_camera(rt["ext"][:, None, :].expand(1, VIEWS, 3), draws[..., 0], draws[..., 1], SIZE)
        return rt, SH.procedural_shell(tables, rt["ext"]).contiguous(), K, Rm, t

    rt, shell_v, K, Rm, t = prepare()
    lib = L.lib()

    def raster(faces):
        L.check(lib.sln_raster_forward(L.ptr(faces), VIEWS, r.F, SIZE, r.near, r.far, L.ptr(r._raster_ws), L.ptr(r.face_index), L.ptr(r._weight),
                                       L.ptr(r._raster_depth), L.current_stream_ptr()), "sln_raster_forward")

    def aten():
        rt, shell_v, K, Rm, t = prepare()
        fx, fl = SH.place_project_torch(tables, rt, shell_v, K, Rm, t, SIZE, r.near)
        raster(fx)
        lab, dep, sums, counts = SH.compose_torch(r.face_index, r._raster_depth, fl, VIEWS)
        chosen, _ = SH.choose_view(sums.reshape(1, VIEWS), counts.reshape(1, VIEWS))
        return lab[chosen], dep[chosen]

    variants = [("ATen composition", aten), ("ViewRenderer", lambda: r(boxes, angles, objs, rows, draws=draws)), ("per-row tables", prepare),
                ("place + project", lambda: SH.place_project(tables, rt, shell_v, K, Rm, t, SIZE, r.near, r.faces_xyz, r.face_label)),
                ("sln_raster_forward", lambda: raster(r.faces_xyz)),
                ("compose", lambda: SH.compose(r.face_index, r._raster_depth, r.face_label, VIEWS, r._compose_ws, r.labels_all, r.depth_all, r.sums, r.counts))]
    lab, dep = aten()
    torch.cuda.synchronize()
    print("   [check] class images of the two routes differ in %d of %d pixels" % (int((lab[0] != r.labels[0]).sum()), SIZE * SIZE))
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window(fn))
    p50 = {}
    for name, _ in variants:
        v = sorted(times[name])
        p50[name] = v[len(v) // 2]
        print("   %-20s %10.1f us  [%9.1f .. %9.1f]   x%6.2f of the ATen composition" % (name, p50[name] * 1e6, v[0] * 1e6, v[-1] * 1e6,
                                                                                        p50["ATen composition"] / p50[name]), flush=True)
    print("   sln_raster_forward is %.1f %% of the ViewRenderer call" % (100 * p50["sln_raster_forward"] / p50["ViewRenderer"]))


if __name__ == "__main__":
    main()
