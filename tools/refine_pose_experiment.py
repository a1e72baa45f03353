"""The synthetic experiment of DESIGN §4 "Camera poses of the target views": targets rendered through known cameras, the loop started from
those cameras with view 1 of every room turned by 0.02 rad and moved by 0.02, ITERS iterations (default 60) of RefineBatch with the poses
held (both steps 0) and with the poses refined, at train.py's defaults, 256 x 256, the rooms and the over-fitted model of
tools/refine_batch_time.py.  Prints, per setting: first and last loss, the pose error of view 1 (angle in rad, distance of the camera
centres; mean and worst room) before and after, the same for view 0 (which starts exact), the mean |boxes - ground truth| of the last
iterate and the size of the recorded gradients.  GPU box.
  ROOMS=4 VIEWS=2 ITERS=60 STEPS="1e-6:1e-6,1e-5:1e-5" python tools/refine_pose_experiment.py"""
import importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
T = importlib.import_module("refine_batch_time")
R, M, syn, RP = T.R, T.M, T.syn, T.RP


def main():
    iters, nr, V = int(os.environ.get("ITERS", "60")), int(os.environ.get("ROOMS", "4")), int(os.environ.get("VIEWS", "2"))
    steps = [tuple(float(x) for x in s.split(":")) for s in os.environ.get("STEPS", "1e-6:1e-6,1e-5:1e-5,1e-4:1e-4").split(",")]
    torch.manual_seed(1)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode='feedforward',
                            gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    l = syn.overfit_to_rooms(model, T.bench_rooms(64)[0], steps=int(os.environ.get("OVERFIT_STEPS", "400")))
    print("over-fitted to 64 rooms: losses [bbox, angle, KL, total] =", [round(float(x), 4) for x in l], flush=True)
    rooms, names = T.bench_rooms(nr)
    bank = R.MeshBank(names, "cuda", seed=3)
    views = T.room_views(rooms, V)
    Rm, t = views[1].double().clone(), views[2].double().clone()
    om = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64) * 0.02
    ta = torch.tensor([-0.48, 0.64, 0.6], dtype=torch.float64) * 0.02
    Rm[:, 1], t[:, 1] = RP.pose_step_torch(Rm[:, 1], t[:, 1], om, ta)
    gt = torch.cat([rm["boxes"][:-1] for rm in rooms])
    fmt = lambda e: "view 1 %.5f / %.5f (worst %.5f / %.5f), view 0 %.5f / %.5f" % (float(e[0][:, 1].mean()), float(e[1][:, 1].mean()), float(e[0][:, 1].max()),
                                                                                    float(e[1][:, 1].max()), float(e[0][:, 0].mean()), float(e[1][:, 0].mean()))
    for rot, trans in [(0.0, 0.0)] + steps:
        rb = R.RefineBatch(model, rooms, bank=bank, iters=iters, views=views, poses=dict(rot_step=rot, trans_step=trans, start=(Rm, t)))
        before = rb.pose_error(views[1], views[2])
        losses = rb.run().cpu()
        after = rb.pose_error(views[1], views[2])
        boxes = torch.cat([b[:-1] for b, _ in rb.results()])
        g = rb.pose_grad
        print("rot_step %g trans_step %g: loss %.4f -> %.4f (mean over %d rooms), finite %s\n   pose error (rad / distance) before: %s\n   after %d iterations:"
              "                  %s\n   mean |boxes - ground truth| %.5f;  |d omega| mean %.3g max %.3g, |d tau| mean %.3g max %.3g" %
              (rot, trans, float(losses[0].mean()), float(losses[-1].mean()), nr, bool(torch.isfinite(losses).all()), fmt(before), iters, fmt(after),
               float((boxes - gt).abs().mean()), float(g[..., :3].norm(dim=-1).mean()), float(g[..., :3].norm(dim=-1).max()),
               float(g[..., 3:].norm(dim=-1).mean()), float(g[..., 3:].norm(dim=-1).max())), flush=True)
        rb.close()
    rb = R.RefineBatch(model, rooms, bank=bank, iters=iters, views=views)
    losses = rb.run().cpu()
    boxes = torch.cat([b[:-1] for b, _ in rb.results()])
    print("exact cameras, poses=None: loss %.4f -> %.4f, mean |boxes - ground truth| %.5f" %
          (float(losses[0].mean()), float(losses[-1].mean()), float((boxes - gt).abs().mean())), flush=True)
    rb.close()


if __name__ == "__main__":
    main()
