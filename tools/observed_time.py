"""Timing of the observed-target builder (GPU box): 16 rooms at 256 x 256, device events.

    python tools/observed_time.py [repeats]

  * the builder alone: ``ObservedTarget`` (csrc/observed_target.hip, two launches) beside ``observed_target_torch`` (the ATen
    restatement) on the same device tensors - p50 and spread over `repeats` windows of ITERS calls, the variants alternated; the bytes
    the work moves by its definition (depth twice - statistics and compose - labels 41 + 1 times, 70 planes written) over the time as
    a fraction of the HBM peak (8.0 TB/s datasheet; a float4 copy reaches 6.29)
  * the constructor of ``RefineBatch`` for the same 16 rooms with and without ``observed=``: the set-up a refinement pays once

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
OB = importlib.import_module("3d_sln_amd.host.observe")
RF = importlib.import_module("3d_sln_amd.host.refine")

HBM_PEAK = 8.0e12
ITERS = int(os.environ.get("ITERS", "20"))
B, S, NCH = 16, 256, 70


def window(fn, iters=ITERS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("observed_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    from oracle import vae_ref
    from test_refine_gpu import FURN, _random_rooms, _room_model
    cfg = vae_ref.VaeConfig()
    model, _ = _room_model(cfg)
    rooms = _random_rooms(B, cfg, seed=3)
    bank = RF.MeshBank(FURN, "cuda", seed=3)
    with torch.no_grad():
        scenes = [RF.RefineScene(rm["class_names"], bank, rm["boxes"][-1].detach().clone(), S) for rm in rooms]
        render = torch.cat([sc.render(rm["boxes"], rm["angles"].float())[0] for sc, rm in zip(scenes, rooms)], 0)
    depth, labels = OB.observe(render)
    chan, dch = scenes[0].chan, scenes[0].dch
    ot = OB.ObservedTarget(chan, dch, S, batch=B)
    got, status = ot(depth, labels)
    want, want_status = OB.observed_target_torch(depth, labels, chan, dch)
    print("observed targets, %d rooms x %d x %d x %d; %d windows of %d calls, device events; p50 [min .. max]" % (B, NCH, S, S, repeats, ITERS))
    print("   [check] elements that differ from the restatement: %d, status %s / %s; from the scene pass's render: plane 0 %d, depth-hot %d" % (
        int((got != want).sum()), status.tolist() == want_status.tolist(), sorted(set(status.tolist())),
        int((got[:, 0] != render[:, 0]).sum()), int((got[:, 41:] != render[:, 41:]).sum())))
    n = S * S
    moved = B * n * (2 * 4 + 42 * 1 + NCH * 4)
    variants = [("observed_target_torch (ATen)", lambda: OB.observed_target_torch(depth, labels, chan, dch), None),
                ("ObservedTarget", lambda: ot(depth, labels), moved)]
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(repeats):
        for name, fn, _ in variants:
            times[name].append(window(fn))
    base = None
    for name, _, nbytes in variants:
        v = sorted(times[name])
        p50 = v[len(v) // 2]
        base = p50 if nbytes is None else base
        line = "   %-32s %9.1f us  [%8.1f .. %8.1f]   x%6.1f" % (name, p50 * 1e6, v[0] * 1e6, v[-1] * 1e6, base / p50)
        if nbytes:
            line += "   %6.1f MB to move (%.1f written), %6.3f TB/s = %4.1f %% of the HBM peak" % (
                nbytes / 1e6, B * n * NCH * 4 / 1e6, nbytes / p50 / 1e12, 100 * nbytes / p50 / HBM_PEAK)
        print(line, flush=True)
    # the constructor's set-up, with and without observed= (one warm-up construction each: tables per geometry are cached)
    kw = dict(bank=bank, learning_rate=1e-3, image_size=S, iters=4)
    setups = [("RefineBatch(...)", {}), ("RefineBatch(..., observed=)", dict(observed=(depth, labels)))]
    times = {name: [] for name, _ in setups}
    for name, extra in setups:
        RF.RefineBatch(model, rooms, **kw, **extra).close()
    for _ in range(max(repeats // 2, 3)):
        for name, extra in setups:
            made = []
            times[name].append(window(lambda: made.append(RF.RefineBatch(model, rooms, **kw, **extra)), iters=1))
            made[0].close()
    for name, _ in setups:
        v = sorted(times[name])
        print("   %-32s %9.2f ms  [%8.2f .. %8.2f]   constructor, device events around it" % (name, v[len(v) // 2] * 1e3, v[0] * 1e3, v[-1] * 1e3), flush=True)


if __name__ == "__main__":
    main()
