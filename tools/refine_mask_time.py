"""Timing of the refinement loss's validity mask (GPU box): 16 rooms at 256 x 256, device events.

    python tools/refine_mask_time.py [repeats]

  * a ``RefineBatch`` iteration of the 16 rooms without ``mask=`` (the launches and bits of before the mask existed) beside the same
    iteration with a mask of 5 % random holes and a rectangle per room - p50 and spread over `repeats` windows of ITERS iterations, the
    two alternated window by window in one process
  * the loss forward + backward alone (``sln_refine_loss_forward`` / ``_backward`` on the batch's image), the same way
  * the set-up call ``sln_refine_loss_mask`` alone (four launches), and the constructor of ``RefineBatch`` with and without ``mask=``

Nothing here is asserted anywhere.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RF = importlib.import_module("3d_sln_amd.host.refine")
_lib = importlib.import_module("3d_sln_amd._lib")

ITERS = int(os.environ.get("ITERS", "20"))
B, S = 16, 256


def window(fn, iters=ITERS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def alternate(variants, repeats, unit=1e6, what="us"):
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window(fn))
    base = None
    for name, _ in variants:
        v = sorted(times[name])
        p50 = v[len(v) // 2]
        base = p50 if base is None else base
        print("   %-44s %9.1f %s  [%8.1f .. %8.1f]   x%6.3f of the first" % (name, p50 * unit, what, v[0] * unit, v[-1] * unit, p50 / base), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("refine_mask_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    from oracle import vae_ref
    from test_refine_gpu import FURN, _random_rooms, _room_model
    cfg = vae_ref.VaeConfig()
    model, _ = _room_model(cfg)
    rooms = _random_rooms(B, cfg, seed=3)
    bank = RF.MeshBank(FURN, "cuda", seed=3)
    rng = np.random.default_rng(7)
    mask = (rng.random((B, S, S)) >= 0.05).astype(np.uint8)
    mask[:, 80:150, 60:200] = 0
    mask = torch.from_numpy(mask).cuda()
    kw = dict(bank=bank, learning_rate=1e-3, image_size=S, iters=4)
    # (the noise of every iteration is drawn at construction and a device counter walks its rows: built for all the iterations timed)
    long = dict(kw, iters=(repeats + 3) * ITERS + 8)
    plain, masked = RF.RefineBatch(model, rooms, **long), RF.RefineBatch(model, rooms, mask=mask, **long)
    for rb in (plain, masked):
        rb.run(1)                                                  # the first iterate's sizes, lazy kernel attributes
    torch.cuda.synchronize()
    cnt = masked.loss.mask_count.cpu()
    print("validity mask, %d rooms x %d x %d; %d windows of %d iterations, device events; p50 [min .. max]" % (B, S, S, repeats, ITERS))
    print("   [check] valid image pixels %.1f %%, valid pooled pixels %.1f %% of %d per room; mask_status %s; losses finite: %s" % (
        100.0 * float(cnt[1].float().mean()) / (S * S), 100.0 * float(cnt[0].float().mean()) / (4 * 96 * 96), 4 * 96 * 96,
        sorted(set(masked.mask_status.tolist())), bool(torch.isfinite(masked.losses[0]).all() and torch.isfinite(plain.losses[0]).all())))
    step = lambda rb: (lambda: rb.run(1))
    alternate([("RefineBatch iteration", step(plain)), ("RefineBatch iteration, mask=", step(masked))], repeats, 1e3, "ms")
    L, P = _lib.lib(), _lib.ptr

    def loss_only(rb):
        rl = rb.loss

        def fn():
            st = _lib.current_stream_ptr()
            L.sln_refine_loss_forward(rl.desc, P(rb.image), P(rl.target_depth), P(rl.labels), P(rl.inv_count), P(rl.ws), P(rb.loss_out), st)
            L.sln_refine_loss_backward(rl.desc, P(rl.ws), P(rb.one), P(rb.g_image), st)
        return fn
    alternate([("loss forward + backward", loss_only(plain)), ("loss forward + backward, mask=", loss_only(masked))], repeats)
    # the set-up call alone, on buffers of its own (the batch's stay as they are)
    rl = masked.loss
    lab, vp, inv = rl.labels.clone(), torch.empty_like(rl.valid_pooled), torch.empty_like(rl.inv_count)
    cnt_d, stat, ws = torch.empty_like(rl.mask_count), torch.empty_like(rl.mask_status), torch.empty_like(rl.ws)
    alternate([("sln_refine_loss_mask (4 launches)",
                lambda: L.sln_refine_loss_mask(rl.desc, P(rl.valid), P(lab), P(vp), P(inv), P(cnt_d), P(stat), P(ws), _lib.current_stream_ptr()))], repeats)
    plain.close(); masked.close()
    setups = [("RefineBatch(...)", {}), ("RefineBatch(..., mask=)", dict(mask=mask))]
    times = {name: [] for name, _ in setups}
    for _ in range(max(repeats // 2, 3)):
        for name, extra in setups:
            made = []
            times[name].append(window(lambda: made.append(RF.RefineBatch(model, rooms, **kw, **extra)), iters=1))
            made[0].close()
    for name, _ in setups:
        v = sorted(times[name])
        print("   %-44s %9.2f ms  [%8.2f .. %8.2f]   constructor, device events around it" % (name, v[len(v) // 2] * 1e3, v[0] * 1e3, v[-1] * 1e3), flush=True)


if __name__ == "__main__":
    main()
