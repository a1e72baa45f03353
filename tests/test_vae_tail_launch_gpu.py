"""The ONE wgrad launch of a full VAE training iteration (run with -m gpu on an MI355X).

A full iteration defers every wgrad to the end of the backward pass.  They used to run as two launches - plain input rows, gathered
input rows - and run as one now, whose workgroups pick the body their problem needs; `SLN_TN_MIXED=0` (read when the engine is
created) restores the two launches in the same build, and the test hook `sln_debug_vae_tail_launches` tells which of the two an
engine issued.  The items, their row chunks and their atomics are the same on both routes.

Bounds (those of tests/test_vae_leaf_launch_gpu.py, whose helpers this file uses): what carries no float atomics - the losses, the
BatchNorm buffers - must agree bit for bit; the gradients within 4 x the spread two runs of the switched-off sequence show against
each other on the same inputs plus 4 ulp of the tensor's largest entry (`_same_gradients` there says why one pair's spread alone
is not a bound)."""
import numpy as np
import pytest
import torch

import test_vae_leaf_launch_gpu as LL
from oracle import vae_ref

pytestmark = pytest.mark.gpu

BASE, LR, ULP = LL.BASE, LL.LR, LL.ULP


def _tail_count(m):
    return int(LL._lib().lib().sln_debug_vae_tail_launches(m._eng))


def _run(cfg, sd, batches, eps, env=None, use_graph=False, two_halves=False):
    """One model, one step per batch under the environment `env` (read when the first step creates the engine).  Per step:
    (losses, {name: gradient}); at the end the BatchNorm buffers and the engine's launch counts."""
    with LL._environ(**(env or {})):
        m = LL._model(cfg, sd).train()
        s = torch.cuda.Stream()
        steps = []
        with torch.cuda.stream(s):
            for b in batches:
                if two_halves:
                    l = m.train_step_begin(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=use_graph)
                    m.train_step_finish(use_graph=use_graph)
                else:
                    l = m.train_step(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=use_graph, with_adam=False)
                s.synchronize()
                steps.append((l.cpu().numpy().copy(), {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}))
        bufs = {k: v.cpu().numpy().copy() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
        return dict(steps=steps, bufs=bufs, tail=_tail_count(m), leaf=LL._leaf_count(m), bn=LL._bn_param_names(m))


OFF = dict(SLN_TN_MIXED="0")
ON = dict(SLN_TN_MIXED=None)


# ------------------------------------------------------------------------------------------- merged against switched off
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_one_launch_gives_the_two_launch_step(use_graph):
    """Two steps on two batches of 4 graphs x (8 objects, 12 triples), eager and replayed."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = LL._batches(cfg, (3, 4))
    eps = LL._eps(cfg, batches[0][0].shape[0])
    u1 = _run(cfg, sd, batches, eps, OFF, use_graph)
    u2 = _run(cfg, sd, batches, eps, OFF, use_graph)
    mg = _run(cfg, sd, batches, eps, ON, use_graph)
    noise = LL._noise(u1, u2)
    print("run-to-run spread of the two-launch sequence: %.3e; one launch vs two: %.3e" % (noise, LL._noise(mg, u1)))
    assert u1["tail"] == 0 and u2["tail"] == 0, "SLN_TN_MIXED=0 must keep one launch per kind"
    assert mg["tail"] == (1 if use_graph else 2), "one mixed launch per issued (or captured) iteration"
    assert mg["leaf"] == u1["leaf"] == (1 if use_graph else 2), "the leaf launch does not depend on the switch"
    LL._same_gradients(mg, u1, noise, "one launch", exact=set(mg["bn"]))
    LL._same_buffers(mg, u1, "one launch")


@pytest.mark.parametrize("mode", ["1", "2"])
def test_the_launch_part_by_part(mode):
    """`SLN_TN_MIXED=1`: the wgrads alone share a launch, the leaf jobs keep theirs; `=2`: the leaf jobs ride behind the wgrads,
    the decoder's assembly backward stays in the chain.  Replayed, against the switched-off sequence."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = LL._batches(cfg, (3, 4))
    eps = LL._eps(cfg, batches[0][0].shape[0])
    u1 = _run(cfg, sd, batches, eps, OFF, True)
    u2 = _run(cfg, sd, batches, eps, OFF, True)
    mg = _run(cfg, sd, batches, eps, dict(SLN_TN_MIXED=mode), True)
    noise = LL._noise(u1, u2)
    print("SLN_TN_MIXED=%s: spread %.3e, against two launches %.3e" % (mode, noise, LL._noise(mg, u1)))
    assert mg["tail"] == 1 and mg["leaf"] == 1
    LL._same_gradients(mg, u1, noise, "SLN_TN_MIXED=" + mode, exact=set(mg["bn"]))
    LL._same_buffers(mg, u1, "SLN_TN_MIXED=" + mode)


def test_deferred_decoder_tables_against_fp64():
    """The decoder's object and attribute tables come out of a job at the very end of the iteration, from a buffer the encoder's
    backward pass must not touch, and the latent gradient reads that buffer's z columns in place: every embedding table and the
    encoder's mean / log-variance Linears (which see the latent gradient first) at 1e-4 of the fp64 oracle, three layers."""
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=3)
    sd = LL._threshold_free(cfg, seed=3)
    cpu = list(vae_ref.synth_batch(4, 8, 12, seed=0, cfg=cfg)[:5])
    eps = torch.from_numpy(np.random.default_rng(1).standard_normal((cpu[0].shape[0], cfg.embedding_dim)).astype(np.float32))
    g64, cpu = LL._fp64_step(cfg, sd, cpu, eps)
    run = _run(cfg, sd, [[t.cuda() for t in cpu]], eps.cuda(), ON)
    assert run["tail"] == 1 and run["leaf"] == 1
    got = run["steps"][0][1]
    keys = [k for k in got if "embedding" in k] + [k for k in got if k.startswith(("box_mean.", "box_var.", "angle_mean.", "angle_var."))]
    assert sum("embedding" in k for k in keys) == 9 and len(keys) > 9, keys
    LL._against_fp64(got, g64, keys, "tail launch")


def test_a_batch_without_triples():
    """No triple rows: the triple-side problems drop out of the list, the object-side ones still share one launch."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=6)
    batches = LL._batches(cfg, (5,))
    batches[0][1] = batches[0][1][:0].contiguous()
    eps = LL._eps(cfg, batches[0][0].shape[0])
    u1 = _run(cfg, sd, batches, eps, OFF)
    u2 = _run(cfg, sd, batches, eps, OFF)
    mg = _run(cfg, sd, batches, eps, ON)
    noise = LL._noise(u1, u2)
    print("no triples: spread %.3e, one launch vs two %.3e, mixed launches %d" % (noise, LL._noise(mg, u1), mg["tail"]))
    assert u1["tail"] == 0 and mg["tail"] == 1
    LL._same_gradients(mg, u1, noise, "no triples", exact=set(mg["bn"]))
    LL._same_buffers(mg, u1, "no triples")


# ------------------------------------------------------------------------------------------- fall-backs
FALLBACKS = {
    "deterministic": dict(det=True),
    "recurrent": dict(cfg=dict(gconv_mode="recurrent")),
    "two_halves": dict(two_halves=True),
    "no_merge": dict(env=dict(SLN_NO_MERGE="1")),
    "leaf_merge_off": dict(env=dict(SLN_LEAF_MERGE="0")),
    "one_flush_off": dict(env=dict(SLN_TN_ONE_FLUSH="0")),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallbacks_keep_one_launch_per_kind(name):
    """Deterministic mode, shared ('recurrent') weights, the two-half data-parallel form and the switches that restore older
    launch sequences never take the mixed launch: no such launch is counted, and the step is the one `SLN_TN_MIXED=0` gives
    (bit for bit, twice, in deterministic mode).  (The sixth listed fall-back, a recorded room group, has the test below.)"""
    f = FALLBACKS[name]
    cfg = vae_ref.VaeConfig(**dict(BASE, **f.get("cfg", {})))
    sd = vae_ref.init_state(cfg, seed=6)
    batches = LL._batches(cfg, (5,))
    eps = LL._eps(cfg, batches[0][0].shape[0])
    env, det, halves = f.get("env", {}), f.get("det", False), f.get("two_halves", False)
    L = LL._lib().lib()
    try:
        L.sln_set_deterministic(int(det))
        u1 = _run(cfg, sd, batches, eps, dict(env, **OFF), two_halves=halves)
        u2 = _run(cfg, sd, batches, eps, dict(env, **OFF), two_halves=halves)
        d1 = _run(cfg, sd, batches, eps, dict(env, **ON), two_halves=halves)
    finally:
        L.sln_set_deterministic(0)
    noise = LL._noise(u1, u2)
    print("%s: run-to-run spread %.3e, default vs SLN_TN_MIXED=0 %.3e" % (name, noise, LL._noise(d1, u1)))
    assert d1["tail"] == 0 and u1["tail"] == 0, "the mixed launch must not be used"
    assert d1["leaf"] == u1["leaf"]
    LL._same_gradients(d1, u1, noise, name, exact=set(d1["bn"]), ordered=det)
    LL._same_buffers(d1, u1, name)
    if det:
        assert noise == 0.0, "deterministic mode: two runs differ"


def _group_run(env, R=3):
    """A recorded room group (host/refine.py::RefineBatch: R engines, created under `env`, whose decoder passes were recorded
    once and run as one launch program): decoder forward, backward, backward.  -> what the group leaves and its engines' counts."""
    import test_hardening_gpu as HG
    L = LL._lib()
    lib = L.lib()
    with LL._environ(**env):
        rb = LL.pkg("host.refine").RefineBatch(HG._model(), HG._rooms(R), image_size=96, iters=3)
    try:
        st = L.current_stream_ptr()
        p0 = rb.params.clone()
        L.check(lib.sln_vae_group_decoder(rb._group, st), "group forward")
        HG._upstream(rb)
        L.check(lib.sln_vae_group_decoder_backward(rb._group, st), "group backward")
        L.check(lib.sln_vae_group_decoder_backward(rb._group, st), "group backward 2")
        torch.cuda.synchronize()
        return dict(dz=rb.dz.cpu().numpy().copy(), boxes=rb.boxes_pred.cpu().numpy().copy(), angles=rb.angles_pred.cpu().numpy().copy(),
                    step=(rb.params - p0).cpu().numpy().copy(), grads=rb.grads.cpu().numpy().copy(),
                    tail=[int(lib.sln_debug_vae_tail_launches(e[0])) for e in rb._engines],
                    leaf=[int(lib.sln_debug_vae_leaf_launches(e[0])) for e in rb._engines])
    finally:
        rb.close()


def test_a_recorded_room_group_keeps_its_own_launch_program():
    """The engines of a room group record their decoder passes (`rec` set, outside train_iteration) and the group replays the
    recorded wgrad flushes through launches of its own: no member engine, created with the default `SLN_TN_MIXED`, ever counts a
    mixed launch or a leaf launch, and what the group computes - outputs and dz bit for bit (no atomics on that path), the fused
    parameter steps and the remaining gradients within 4 x the spread of two `SLN_TN_MIXED=0` groups + 4 ulp of the largest entry -
    is what the same group built with `SLN_TN_MIXED=0` computes."""
    u1, u2, on = _group_run(OFF), _group_run(OFF), _group_run(ON)
    for run, what in ((u1, "SLN_TN_MIXED=0"), (on, "default")):
        assert run["tail"] == [0] * len(run["tail"]) and run["leaf"] == [0] * len(run["leaf"]), "%s: %s" % (what, run)
    for k in ("dz", "boxes", "angles"):
        assert np.array_equal(on[k], u1[k]), k
    assert float(np.abs(on["step"]).max()) > 0.0
    for k in ("step", "grads"):
        scale = float(np.abs(u1[k]).max())
        spread = float(np.abs(u1[k] - u2[k]).max())
        d = float(np.abs(on[k] - u1[k]).max())
        print("room group %s: scale %.3e, two switched-off groups %.3e apart, default vs switched off %.3e" % (k, scale, spread, d))
        assert d <= 4.0 * spread + 4.0 * ULP * scale, (k, d, spread, scale)


# ------------------------------------------------------------------------------------------- with Adam
def test_three_adam_steps_one_launch_against_two():
    """Three replayed steps with the optimizer, the three models in lockstep as in
    test_vae_leaf_launch_gpu.py::test_three_adam_steps_merged_against_unmerged (which explains the bounds): before steps 2 and 3
    the two others take over the first model's parameters, BatchNorm buffers and Adam moments."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = LL._batches(cfg, (3, 4, 5))
    eps = LL._eps(cfg, batches[0][0].shape[0])
    models = {name: LL._model(cfg, sd).train() for name in ("u1", "u2", "mg")}
    s = torch.cuda.Stream()
    bad = []
    with torch.cuda.stream(s):
        for i, b in enumerate(batches):
            st, losses = {}, {}
            for name, m in models.items():
                if i > 0 and name != "u1":
                    m.load_state_dict(models["u1"].state_dict())
                    m._adam_m.copy_(models["u1"]._adam_m); m._adam_v.copy_(models["u1"]._adam_v)
                    assert torch.equal(m.flat_params, models["u1"].flat_params)
                s.synchronize()
            for name, m in models.items():
                with LL._environ(**(ON if name == "mg" else OFF)):
                    l = m.train_step(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=True)
                s.synchronize()
                st[name], losses[name] = LL._state(m), l.cpu().numpy().copy()
            assert np.array_equal(losses["mg"], losses["u1"]), "step %d: same parameters, same forward" % i
            gmax = max(float(np.abs(v).max()) for v in st["u1"]["grads"].values())
            residue = {k for k, v in st["u1"]["grads"].items() if float(np.abs(v).max()) < 1e-6 * gmax}
            for q in ("grads", "adam_m", "adam_v", "params"):
                a, b2, g = st["u1"][q], st["u2"][q], st["mg"][q]
                floor = 1e-6 * max(float(np.abs(v).max()) for v in a.values())
                scale = {k: max(float(np.abs(v).max()), floor) for k, v in a.items()}
                keys = [k for k in a if not (q == "params" and k in residue)]
                spread = max(float(np.abs(a[k] - b2[k]).max()) / scale[k] for k in keys)
                worst = max(float(np.abs(g[k] - a[k]).max()) / scale[k] for k in keys)
                print("step %d %-7s two launches run-to-run %.3e, one launch vs two %.3e" % (i, q, spread, worst))
                for k in a:
                    d = float(np.abs(g[k] - a[k]).max())
                    if q == "params" and k in residue:
                        bound = 2.02 * LR
                    else:
                        bound = (4.0 * spread + 4.0 * ULP + (2.0 * ULP if q == "params" else 0.0)) * scale[k]
                    if d > bound:
                        bad.append("step %d %s %s: differs by %.3e (bound %.3e)" % (i, q, k, d, bound))
    assert _tail_count(models["mg"]) == 1 and _tail_count(models["u1"]) == 0 and _tail_count(models["u2"]) == 0
    assert not bad, "\n".join(bad[:30])
