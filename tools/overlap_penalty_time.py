"""Timing of the interpenetration penalty in the R-rooms-in-flight refinement loop (RefineBatch(overlap_weight=)), tools/refine_batch_time.py's
rooms at train.py's defaults, 256 x 256.  GPU box.

    python tools/overlap_penalty_time.py loop [--rooms 16,64] [--weight 0.0] [--iters 30] [--tree DIR]
        ms per iteration (slope between runs of ITERS and 2 x ITERS iterations, median of three pairs), one JSON line.  --tree: the checkout whose
        package is measured (default: this one; a checkout without the feature can only take --weight 0).
    python tools/overlap_penalty_time.py compare --other DIR [--rounds 4] [--rooms 16,64] [--weight-on 0.05]
        `loop` with the weight at 0 in fresh processes, this checkout and the (built) checkout of the parent commit at DIR alternated, then this
        checkout with the weight on: is the weight-0 figure inside the parent's own run-to-run spread, and what does the penalty cost.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o e -- python tools/overlap_penalty_time.py kernel [--rooms 16,64]
        sln_layout_overlap_penalty alone on one layout of R rooms of 13 rows as the loop calls it (a run of its own: the kernel's time is in
        OUT/**/e_kernel_stats.csv).
"""
import argparse
import importlib
import inspect
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _package(tree):
    sys.path.insert(0, tree)
    import torch
    return (torch, importlib.import_module("3d_sln_amd.host.refine"), importlib.import_module("3d_sln_amd.host.Sg2ScVAE_model"),
            importlib.import_module("3d_sln_amd.host.synthetic"))


def bench_rooms(torch, n_rooms, n_obj=12, seed=0, dev="cuda"):
    """the rooms of tools/refine_batch_time.py"""
    names = ["bed", "chair", "table", "sofa", "desk", "cabinet", "lamp", "television", "bookshelf", "dresser", "night_stand", "shelves"]
    rooms = []
    for r in range(n_rooms):
        g = torch.Generator().manual_seed(seed + r)
        cn = names[:n_obj] + ["__room__"]; n = len(cn)
        lo = torch.rand(n, 3, generator=g) * 0.45 + 0.05; lo[:, 1] = 0.0; lo[:, 2] *= 0.6
        hi = lo + torch.rand(n, 3, generator=g) * 0.2 + 0.12
        boxes = torch.cat([lo, hi], 1); boxes[-1] = torch.tensor([0, 0, 0, 4.0, 2.7, 5.0])
        objs = torch.arange(1, n + 1); objs[-1] = 0
        tri = torch.tensor([[i, 1 + i % 10, (i + 1) % (n - 1)] for i in range(n - 1)] + [[i, 0, n - 1] for i in range(n - 1)])
        rooms.append(dict(objs=objs.to(dev), triples=tri.to(dev), boxes=boxes.to(dev), angles=torch.randint(0, 24, (n,), generator=g).to(dev),
                          attributes=torch.zeros(n, dtype=torch.int64, device=dev), class_names=cn))
    return rooms, names


def loop(args):
    torch, R, M, syn = _package(args.tree)
    torch.manual_seed(1)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode='feedforward',
                            gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):                   # a trained checkpoint places the furniture in view; a random decoder renders the empty room
        syn.overfit_to_rooms(model, bench_rooms(torch, 64)[0], steps=args.overfit_steps)
    has = "overlap_weight" in inspect.signature(R.RefineBatch.__init__).parameters
    if args.weight > 0 and not has:
        raise SystemExit("this checkout has no overlap_weight")
    kw = dict(overlap_weight=args.weight) if has else {}
    out = {}
    for nr in args.rooms:
        rooms, names = bench_rooms(torch, nr)
        bank = R.MeshBank(names, "cuda", seed=3)
        res, pen = [], None
        with torch.cuda.stream(st):
            for n_it in (args.iters, 2 * args.iters) * 3:
                rb = R.RefineBatch(model, rooms, bank=bank, iters=n_it, **kw)
                torch.cuda.synchronize(); t1 = time.perf_counter()
                rb.run()
                torch.cuda.synchronize(); t2 = time.perf_counter()
                res.append((n_it, t2 - t1))
                if getattr(rb, "overlap", None) is not None:
                    pen = [float(rb.overlap[0].mean()), float(rb.overlap[n_it - 1].mean())]
                assert bool(torch.isfinite(rb.losses).all())
                rb.close()
        a = statistics.median(t for n, t in res if n == args.iters); b = statistics.median(t for n, t in res if n == 2 * args.iters)
        out[str(nr)] = dict(ms_per_iteration=(b - a) / args.iters * 1e3, mean_penalty_first_last=pen)
    print("RESULT " + json.dumps(dict(tree=args.tree, weight=args.weight, rooms=out)), flush=True)


def _child(tree, weight, args):
    cmd = [sys.executable, os.path.abspath(__file__), "loop", "--tree", tree, "--weight", str(weight), "--iters", str(args.iters),
           "--rooms", ",".join(str(r) for r in args.rooms), "--overfit-steps", str(args.overfit_steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, cwd=tree)
    if r.returncode != 0:
        raise SystemExit("child failed (%d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])["rooms"]


def compare(args):
    runs = {"parent": [], "weight 0": [], "weight on": []}
    for k in range(args.rounds):
        for name, tree, w in (("parent", args.other, 0.0), ("weight 0", HERE, 0.0)):
            runs[name].append(_child(tree, w, args))
            print("round %d %-9s %s" % (k, name, {r: round(v["ms_per_iteration"], 4) for r, v in runs[name][-1].items()}), flush=True)
    for k in range(2):
        runs["weight on"].append(_child(HERE, args.weight_on, args))
        print("weight %g: %s" % (args.weight_on, runs["weight on"][-1]), flush=True)
    for nr in (str(r) for r in args.rooms):
        ms = {name: [x[nr]["ms_per_iteration"] for x in v] for name, v in runs.items()}
        lo, hi, med = min(ms["parent"]), max(ms["parent"]), statistics.median(ms["weight 0"])
        print("rooms %s: parent %.4f .. %.4f ms / iteration (median %.4f); weight 0: %.4f .. %.4f (median %.4f) - %s the parent's spread; "
              "weight %g: %s ms (+%.4f ms on the weight-0 median)"
              % (nr, lo, hi, statistics.median(ms["parent"]), min(ms["weight 0"]), max(ms["weight 0"]), med, "inside" if lo <= med <= hi else "OUTSIDE",
                 args.weight_on, ", ".join("%.4f" % v for v in ms["weight on"]), statistics.median(ms["weight on"]) - med), flush=True)


def kernel(args):
    torch, R, _, _ = _package(args.tree)
    EV = importlib.import_module("3d_sln_amd.host.evaluate")
    for nr in args.rooms:
        rooms, _ = bench_rooms(torch, nr)
        n = int(rooms[0]["objs"].shape[0])
        boxes = torch.cat([rm["boxes"] for rm in rooms]).float()[None].contiguous()
        angles = torch.cat([rm["angles"] for rm in rooms]).float()[None].contiguous()
        rr = torch.cat([torch.full((n,), r * n + n - 1, dtype=torch.int32) for r in range(nr)]).cuda()
        rid = torch.cat([torch.full((n,), r, dtype=torch.int32) for r in range(nr)]).cuda()
        collide = torch.tensor(([1] * (n - 1) + [0]) * nr, dtype=torch.uint8).cuda()
        gb, ga = torch.zeros(1, nr * n, 6, device="cuda"), torch.zeros(1, nr * n, device="cuda")
        pen = torch.zeros(1, nr, dtype=torch.float64, device="cuda")
        for _ in range(args.calls):
            EV.overlap_penalty_launch(boxes, angles, rr, collide, rid, nr, 0.05, True, pen, gb, ga)
        torch.cuda.synchronize()
        print("rooms %d (%d rows): %d calls, mean penalty per room %.4f" % (nr, nr * n, args.calls, float(pen.mean())), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("mode", choices=["loop", "compare", "kernel"])
    p.add_argument("--rooms", type=lambda s: [int(x) for x in s.split(",")], default=[16, 64])
    p.add_argument("--weight", type=float, default=0.0)
    p.add_argument("--weight-on", type=float, default=0.05)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--overfit-steps", type=int, default=400)
    p.add_argument("--tree", default=HERE)
    p.add_argument("--other")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--calls", type=int, default=200)
    args = p.parse_args()
    if args.mode == "compare" and not args.other:
        p.error("compare needs --other DIR: a built checkout of the parent commit")
    args.tree, args.other = os.path.abspath(args.tree), os.path.abspath(args.other) if args.other else None
    {"loop": loop, "compare": compare, "kernel": kernel}[args.mode](args)


if __name__ == "__main__":
    main()
