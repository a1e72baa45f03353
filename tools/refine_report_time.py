"""Timing of the refinement report (GPU box).

  python tools/refine_report_time.py loop [rooms,rooms,...]    RefineBatch at 256 x 256 (the rooms and model of tools/refine_batch_time.py),
        eager: ms per iteration with report=None, "ends" and "all", interleaved and repeated so that the run-to-run spread is on the
        table next to the differences (slope between runs of ITERS and 2 x ITERS iterations, as refine_batch_time.py)
  python tools/refine_report_time.py metrics                   layouts/s of cuboid_iou and layout_overlap at S = 20 000 on one room and on
        a 512-room collated batch (S = 200), beside the float64 torch restatement on the CPU (16 threads)
"""
import importlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
E = importlib.import_module("3d_sln_amd.host.evaluate")


def loop(room_counts):
    import refine_batch_time as T
    R, M, syn = T.R, T.M, T.syn
    iters, reps = int(os.environ.get("ITERS", "60")), int(os.environ.get("REPS", "3"))
    torch.manual_seed(1)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode='feedforward',
                            gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        syn.overfit_to_rooms(model, T.bench_rooms(64)[0], steps=int(os.environ.get("OVERFIT_STEPS", "400")))
    for nr in room_counts:
        rooms, names = T.bench_rooms(nr)
        bank = R.MeshBank(names, "cuda", seed=3)
        with torch.cuda.stream(st):
            def one(report, n_it):
                rb = R.RefineBatch(model, rooms, bank=bank, iters=n_it, report=report)
                torch.cuda.synchronize(); t0 = time.perf_counter()
                rb.run()
                torch.cuda.synchronize(); dt = time.perf_counter() - t0
                rep = rb.report[0, 0].tolist() if report is not None else None
                rb.close()
                return dt, rep
            one(None, iters)                                                # warm-up
            slopes = {None: [], "ends": [], "all": []}
            for _ in range(reps):
                for mode in (None, "ends", "all"):
                    a, _ = one(mode, iters); b, rep = one(mode, 2 * iters)
                    slopes[mode].append((b - a) / iters * 1e3)
            for mode in (None, "ends", "all"):
                v = sorted(slopes[mode])
                print("rooms %2d report=%-5s ms / iteration: median %.4f  (runs: %s)" % (nr, mode, v[len(v) // 2], " ".join("%.4f" % x for x in slopes[mode])),
                      flush=True)
            print("   report[0, 0] of the last run:", rep, flush=True)


def _timed(fn, reps, sync):
    fn(); sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps


def metrics():
    torch.set_num_threads(16)
    gen = torch.Generator().manual_seed(0)
    for n_rooms, per_room, S, S_cpu in ((1, 12, 20000, 2000), (512, 12, 200, 8)):
        O = n_rooms * (per_room + 1)
        lo = torch.rand(O, 3, generator=gen) * 0.6
        gt = torch.cat([lo, lo + 0.1 + 0.3 * torch.rand(O, 3, generator=gen)], 1)
        rr = torch.arange(O, dtype=torch.int32) // (per_room + 1) * (per_room + 1) + per_room
        gt[rr.long() == torch.arange(O)] = torch.tensor([0, 0, 0, 4.0, 2.7, 5.0])
        ga = torch.randint(0, 24, (O,), generator=gen).float()
        boxes = gt[None] + 0.05 * torch.randn(S, O, 6, generator=gen)
        ang = ga[None] + 0.5 * torch.randn(S, O, generator=gen)
        vis = torch.ones(O, dtype=torch.bool)
        d = lambda t: t.cuda()
        B, A, G, GA, RR, V = d(boxes), d(ang), d(gt), d(ga), d(rr), d(vis)
        rid, nrm = E._room_ids(RR)
        mean = torch.zeros(S, nrm, dtype=torch.float64, device="cuda")
        vol, prs = torch.zeros(S, dtype=torch.float64, device="cuda"), torch.zeros(S, dtype=torch.int64, device="cuda")
        t_iou = _timed(lambda: E.cuboid_iou(B, A, G, GA, RR, V, room_id=rid, n_rooms=nrm, want_rows=False, mean=mean), 20, torch.cuda.synchronize)
        t_ov = _timed(lambda: E.layout_overlap(B, A, RR, V, thresh=0.1, vol=vol, pairs=prs), 20, torch.cuda.synchronize)
        c_iou = _timed(lambda: E.cuboid_iou_torch(boxes[:S_cpu], ang[:S_cpu], gt, ga, rr, vis, room_id=rid.cpu(), n_rooms=nrm), 2, lambda: None)
        c_ov = _timed(lambda: E.layout_overlap_torch(boxes[:S_cpu], ang[:S_cpu], rr, vis, 0.1), 2, lambda: None)
        print("%3d room(s), O = %d rows, S = %d layouts (host wall clock per call, wrapper's table checks included):" % (n_rooms, O, S))
        print("   cuboid_iou      %9.1f us  %12.0f layouts/s   | CPU float64 restatement (S = %d): %10.0f layouts/s" % (t_iou * 1e6, S / t_iou, S_cpu, S_cpu / c_iou))
        print("   layout_overlap  %9.1f us  %12.0f layouts/s   | CPU float64 restatement (S = %d): %10.0f layouts/s" % (t_ov * 1e6, S / t_ov, S_cpu, S_cpu / c_ov),
              flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "metrics"
    if what == "loop":
        loop([int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "16,64").split(",")])
    else:
        metrics()
