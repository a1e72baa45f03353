"""Timing of the R-rooms-in-flight refinement loop (host/refine.py::RefineBatch) at train.py's defaults, 256 x 256: ms per iteration
(slope between runs of `iters` and 2 x `iters` iterations) and set-up per room, eager and under hipGraph replay.  GPU box.
VIEWS=V (default 0: ``views=None``): refine every room against V target views - view 0 is ``refine_view``'s camera, the others look from the
room's upper corners at its centre (``look_at_view``).  POSES=1 (needs VIEWS): refine the views' poses as well (``poses=``; ROT_STEP / TRANS_STEP,
default 1e-6 each) - one more launch per iteration, sln_place_pose_step_views.  INTRINSICS=1 (needs VIEWS; with or without POSES): refine
the views' focal lengths and principal points as well (``intrinsics=``; FOCAL_STEP, default 1e-6, CENTER_STEP, default 1e-4) - the one launch
is then sln_place_camera_step_views.  CONFIDENCE=1: the loss under a per-pixel confidence (``confidence=``: bands at 255 / 128 and a rectangle at 0
on every image); MASK=1: under the validity mask on the same support (``mask=``: the confidence's non-zero pixels).  Every line also gives the smallest and the largest of the three slopes (run i of 2 x `iters` against
run i of `iters`)."""
import importlib, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
R = importlib.import_module("3d_sln_amd.host.refine")
M = importlib.import_module("3d_sln_amd.host.Sg2ScVAE_model")
syn = importlib.import_module("3d_sln_amd.host.synthetic")
RP = importlib.import_module("3d_sln_amd.host.reproject")


def bench_rooms(n_rooms, n_obj=12, seed=0, dev="cuda"):
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


_CORNERS = ((0.9, 0.9, 0.9), (0.1, 0.9, 0.9), (0.9, 0.9, 0.1), (0.1, 0.9, 0.1))


def room_views(rooms, V):
    """(K [R, V, 3, 3], Rm, t [R, V, 3]) on the host; None for V = 0"""
    if V < 1:
        return None
    cams = []
    for rm in rooms:
        ext = rm["boxes"][-1, 3:].cpu().double().numpy()
        cams.append([RP.refine_view(rm["boxes"][-1], 256)[:3]] +
                    [RP.look_at_view(ext * _CORNERS[(v - 1) % 4] * (1.0 - 0.1 * ((v - 1) // 4)), ext / 2)[:3] for v in range(1, V)])
    return tuple(torch.stack([torch.stack([c[v][j] for v in range(V)]) for c in cams]) for j in range(3))


def confidence_image(n_images, S=256, dev="cuda"):
    """uint8 [n_images, S, S]: rows in six bands at 255 / 128, a rectangle without a say"""
    band = torch.tensor([255, 128, 255, 128, 128, 255], dtype=torch.uint8)[torch.arange(S) * 6 // S]
    c = band[None, :, None].repeat(n_images, 1, S)
    c[:, S // 4:S // 2, S // 3:2 * S // 3] = 0
    return c.to(dev).contiguous()


def main():
    iters = int(os.environ.get("ITERS", "60"))
    n_views = int(os.environ.get("VIEWS", "0"))
    torch.manual_seed(1)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode='feedforward',
                            gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    st = torch.cuda.Stream()
    if not os.environ.get("NO_OVERFIT"):           # a trained checkpoint places the furniture in view; a random decoder renders the empty room
        with torch.cuda.stream(st):
            l = syn.overfit_to_rooms(model, bench_rooms(64)[0], steps=int(os.environ.get("OVERFIT_STEPS", "400")))
        print("over-fitted to 64 rooms: losses [bbox, angle, KL, total] =", [round(float(x), 4) for x in l], flush=True)
    for nr in [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "1,4,16").split(",")]:
        rooms, names = bench_rooms(nr)
        bank = R.MeshBank(names, "cuda", seed=3)
        views = room_views(rooms, n_views)
        poses = None
        if os.environ.get("POSES", "0") != "0":
            poses = dict(rot_step=float(os.environ.get("ROT_STEP", "1e-6")), trans_step=float(os.environ.get("TRANS_STEP", "1e-6")))
        intrinsics = None
        if os.environ.get("INTRINSICS", "0") != "0":
            intrinsics = dict(focal_step=float(os.environ.get("FOCAL_STEP", "1e-6")), center_step=float(os.environ.get("CENTER_STEP", "1e-4")))
        extra = dict(intrinsics=intrinsics) if intrinsics else {}
        if os.environ.get("CONFIDENCE", "0") != "0" or os.environ.get("MASK", "0") != "0":
            conf = confidence_image(nr * max(n_views, 1)).view(*((nr, n_views) if n_views else (nr,)), 256, 256)
            extra.update(dict(confidence=conf) if os.environ.get("CONFIDENCE", "0") != "0" else dict(mask=(conf != 0).to(torch.uint8)))
            print("rooms %d: %s" % (nr, "confidence=" if "confidence" in extra else "mask="), flush=True)
        with torch.cuda.stream(st):
            for capture in (False, True):
                res = []; enq = []
                for n_it in (iters, 2 * iters, iters, 2 * iters, iters, 2 * iters):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    G = int(os.environ.get("GROUPS", "1"))
                    rb = R.RefineBatch(model, rooms, bank=bank, iters=n_it, views=views, poses=poses, **extra)
                    torch.cuda.synchronize(); t1 = time.perf_counter()
                    rb.run(capture=capture)
                    t_enq = time.perf_counter() - t1                  # host time to enqueue everything (the GPU may still be running)
                    torch.cuda.synchronize(); t2 = time.perf_counter()
                    enq.append(t_enq / n_it)
                    lv = rb.live.cpu(); live = (float((lv == 3).sum()) / lv.shape[0], float((lv == 1).sum()) / lv.shape[0])
                    res.append((n_it, t1 - t0, t2 - t1)); info = rb.launches(); fin = bool(torch.isfinite(rb.losses).all()); rb.close()
                a = sorted(x[2] for x in res if x[0] == iters)[1]; b = sorted(x[2] for x in res if x[0] == 2 * iters)[1]
                setup = sorted(x[1] for x in res)[len(res) // 2]
                slopes = [(res[i + 1][2] - res[i][2]) / iters * 1e3 for i in (0, 2, 4)]
                print("rooms %2d views %d%s%s %s: %.3f ms / iteration (min-max of the three slopes %.3f-%.3f; %.4f per room-iteration), run-intercept %.2f ms, set-up %.2f ms per room, %s, finite %s"
                      % (nr, n_views, " poses" if poses else "", " intrinsics" if intrinsics else "", "graph" if capture else "eager", (b - a) / iters * 1e3, min(slopes), max(slopes), (b - a) / iters * 1e3 / nr, (a - (b - a)) * 1e3, setup * 1e3 / nr, info, fin), flush=True)
                print("   host enqueue time per iteration: %.3f ms (min over runs); planes per image: %.1f live, %.1f constant" % (min(enq) * 1e3, live[0], live[1]), flush=True)


if __name__ == "__main__":
    main()
