"""The synthetic experiment of DESIGN §4 "Intrinsics of the target views": targets rendered through known cameras, the loop started from those
cameras with the focal lengths of view 1 of every room OFF per cent off (default 3: high), ITERS iterations (default 60) of RefineBatch at
train.py's defaults, 256 x 256, the rooms and the over-fitted model of tools/refine_batch_time.py.  Per focal step of FOCAL_STEPS three runs:

  * intrinsics   the poses exact and held (``poses=None``), the intrinsics free;
  * both         poses and intrinsics free (pose steps ROT_STEP / TRANS_STEP, default 1e-5 each);
  * poses        the poses alone free, K held at the wrong start (focal and centre step 0);

in front of them the run that holds everything at the wrong start, behind them the run with exact cameras and no camera step.  Prints,
per run: first and last loss, the focal error of view 1 and of view 0 (relative; mean and worst room), the distance of the principal
points, the pose error of both views (angle in rad / distance of the camera centres), the mean |boxes - ground truth| of the last iterate,
and for view 1 the mean change of log(focal length) beside the mean change of the camera centre's distance from the room's centre along
the viewing axis, relative to that distance - a focal length and a dolly that trade against each other show up as the two moving together.
GPU box.
  ROOMS=4 VIEWS=2 ITERS=60 FOCAL_STEPS="1e-4,1e-3" CENTER_STEP=0 python tools/refine_intrinsics_experiment.py"""
import importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
T = importlib.import_module("refine_batch_time")
R, M, syn, RP = T.R, T.M, T.syn, T.RP


def main():
    iters, nr, V = int(os.environ.get("ITERS", "60")), int(os.environ.get("ROOMS", "4")), int(os.environ.get("VIEWS", "2"))
    focal_steps = [float(x) for x in os.environ.get("FOCAL_STEPS", "1e-4,1e-3").split(",")]
    center_step, off = float(os.environ.get("CENTER_STEP", "0")), float(os.environ.get("OFF", "3")) / 100.0
    rot, trans = float(os.environ.get("ROT_STEP", "1e-5")), float(os.environ.get("TRANS_STEP", "1e-5"))
    torch.manual_seed(1)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode='feedforward',
                            gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    l = syn.overfit_to_rooms(model, T.bench_rooms(64)[0], steps=int(os.environ.get("OVERFIT_STEPS", "400")))
    print("over-fitted to 64 rooms: losses [bbox, angle, KL, total] =", [round(float(x), 4) for x in l], flush=True)
    rooms, names = T.bench_rooms(nr)
    bank = R.MeshBank(names, "cuda", seed=3)
    views = T.room_views(rooms, V)
    K0 = views[0].double().clone()
    K0[:, 1, 0, 0] *= 1.0 + off
    K0[:, 1, 1, 1] *= 1.0 + off
    gt = torch.cat([rm["boxes"][:-1] for rm in rooms])
    centre = torch.stack([rm["boxes"][-1, 3:].cpu().double() / 2 for rm in rooms])                 # [R, 3]: what the corner views look at

    def depth(Rm, t):
        """the room centre's z in the camera of view 1, [R]"""
        return (Rm[:, 1, 2].cpu() * centre).sum(-1) + t[:, 1, 2].cpu()

    pair = lambda e, v: "%.5f / %.5f (worst %.5f / %.5f)" % (float(e[0][:, v].mean()), float(e[1][:, v].mean()), float(e[0][:, v].max()), float(e[1][:, v].max()))
    runs = [("held at the wrong start", dict(focal_step=0.0, center_step=0.0), None)]
    for fs in focal_steps:
        runs += [("intrinsics, focal step %g" % fs, dict(focal_step=fs, center_step=center_step), None),
                 ("both, focal step %g" % fs, dict(focal_step=fs, center_step=center_step), dict(rot_step=rot, trans_step=trans)),
                 ("poses, focal step %g" % fs, dict(focal_step=0.0, center_step=0.0), dict(rot_step=rot, trans_step=trans))]
    seen = set()
    for name, intr, poses in runs:
        if name.startswith("poses"):                    # (the poses-alone run does not depend on the focal step: once)
            if "poses" in seen:
                continue
            seen.add("poses")
            name = "poses alone"
        rb = R.RefineBatch(model, rooms, bank=bank, iters=iters, views=views, poses=poses, intrinsics=dict(intr, start=K0))
        z0 = depth(*rb.poses())
        losses = rb.run().cpu()
        ek, ep = rb.intrinsics_error(views[0]), rb.pose_error(views[1], views[2])
        K = rb.intrinsics().cpu()
        z1 = depth(*rb.poses())
        boxes = torch.cat([b[:-1] for b, _ in rb.results()])
        dlog = torch.log(K[:, 1, 0, 0] / K0[:, 1, 0, 0])
        print("%s (centre step %g, pose steps %s): loss %.4f -> %.4f (mean over %d rooms), finite %s\n"
              "   focal error / principal point: view 1 %s, view 0 %s\n   pose error (rad / distance):    view 1 %s, view 0 %s\n"
              "   mean |boxes - ground truth| %.5f;  view 1: mean d log f %+.5f, mean relative d depth of the room centre %+.5f (per room: %s / %s)" %
              (name, intr["center_step"], "%g / %g" % (rot, trans) if poses else "-", float(losses[0].mean()), float(losses[-1].mean()), nr,
               bool(torch.isfinite(losses).all()), pair(ek, 1), pair(ek, 0), pair(ep, 1), pair(ep, 0), float((boxes - gt).abs().mean()), float(dlog.mean()),
               float(((z1 - z0) / z0).mean()), [round(float(x), 5) for x in dlog], [round(float(x), 5) for x in (z1 - z0) / z0]), flush=True)
        rb.close()
    rb = R.RefineBatch(model, rooms, bank=bank, iters=iters, views=views)
    losses = rb.run().cpu()
    boxes = torch.cat([b[:-1] for b, _ in rb.results()])
    print("exact cameras, poses=None, intrinsics=None: loss %.4f -> %.4f, mean |boxes - ground truth| %.5f" %
          (float(losses[0].mean()), float(losses[-1].mean()), float((boxes - gt).abs().mean())), flush=True)
    rb.close()


if __name__ == "__main__":
    main()
