"""The VAE training step under the two split words of the wgrad launches (sln_set_tn_split; run with -m gpu on an MI355X).

4 graphs x (8 objects, 12 triples), the helpers of tests/test_vae_leaf_launch_gpu.py.  The word changes how a wgrad sums, nothing else:
  * losses and BatchNorm buffers (no wgrad feeds them) bit for bit between the words;
  * every parameter gradient's distance from the fp64 oracle (oracle/vae_ref.py in double) at most twice the fp32 route's distance
    on the same batch plus 4 ulp of the tensor's largest entry.  The factor is a margin, not a measurement: the split drops 2^-24
    of each product and fp32 accumulation rounds by as much (tests/test_tn_split_host.py), so the two errors are of one order;
  * deterministic mode keeps the fp32 body: the same bits under both words;
  * replays under 0, 0, 1, 1, 0 on one engine: the capture counter steps at the changes only;
  * each fall-back route (SLN_TN_MIXED=0/1/2, SLN_NO_MERGE=1) against the tail launch under word 1, as
    tests/test_vae_tail_launch_gpu.py compares them under the default: within 4 x the run-to-run spread plus 4 ulp;
  * three Adam steps in lockstep from equal states, at the bounds of tests/test_vae_leaf_launch_gpu.py's Adam test; parameter elements
    whose gradient is next to zero are held to Adam's 2 lr instead (see the test)."""
import numpy as np
import pytest
import torch

import test_vae_leaf_launch_gpu as LL
from oracle import vae_ref

pytestmark = pytest.mark.gpu

BASE, LR, ULP = LL.BASE, LL.LR, LL.ULP
F32, SPLIT = 0, 1


@pytest.fixture
def lib():
    h = LL._lib().lib()
    word, det = h.sln_get_tn_split(), h.sln_get_deterministic()
    yield h
    assert h.sln_set_tn_split(word) == 0
    h.sln_set_deterministic(det)


def _run(h, word, cfg, sd, batches, eps, use_graph, env=None):
    assert h.sln_set_tn_split(word) == 0
    with LL._environ(**(env or {})):
        return LL._run(cfg, sd, batches, eps, True, use_graph=use_graph)


def _setup(seeds=(3, 4)):
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = LL._batches(cfg, seeds)
    return cfg, sd, batches, LL._eps(cfg, batches[0][0].shape[0])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_losses_and_buffers_bit_for_bit(lib, use_graph):
    cfg, sd, batches, eps = _setup()
    lib.sln_set_deterministic(0)
    off = _run(lib, F32, cfg, sd, batches, eps, use_graph)
    on = _run(lib, SPLIT, cfg, sd, batches, eps, use_graph)
    for i, ((l1, _), (l0, _)) in enumerate(zip(on["steps"], off["steps"])):
        assert np.array_equal(l1, l0), "step %d: losses %s vs %s" % (i, l1, l0)
    LL._same_buffers(on, off, "split")
    print("split against fp32 wgrads, largest gradient difference / tensor max: %.3e" % LL._noise(on, off))


def test_gradients_against_fp64_next_to_the_fp32_route(lib):
    cfg = vae_ref.VaeConfig(**BASE)
    sd = LL._threshold_free(cfg, seed=3)
    cpu = list(vae_ref.synth_batch(4, 8, 12, seed=0, cfg=cfg)[:5])
    eps = torch.from_numpy(np.random.default_rng(1).standard_normal((cpu[0].shape[0], cfg.embedding_dim)).astype(np.float32))
    g64, cpu = LL._fp64_step(cfg, sd, cpu, eps)
    dev = [[t.cuda() for t in cpu]]
    lib.sln_set_deterministic(0)
    g = {w: _run(lib, w, cfg, sd, dev, eps.cuda(), False)["steps"][0][1] for w in (F32, SPLIT)}
    bad, worst = [], 0.0
    for k in sorted(g[F32]):
        ref = g64[k].numpy() if k in g64 else np.zeros(g[F32][k].shape)
        d0, d1 = (float(np.abs(g[w][k] - ref).max()) for w in (F32, SPLIT))
        scale = float(np.abs(ref).max())
        bound = 2.0 * d0 + 4.0 * ULP * scale
        ratio = d1 / d0 if d0 > 0 else float("nan")
        worst = max(worst, ratio) if d0 > 0 else worst
        print("%-52s fp32 %.3e split %.3e ratio %.2f scale %.3e" % (k, d0, d1, ratio, scale))
        if d1 > bound:
            bad.append("%s: split %.3e from fp64, fp32 %.3e, bound %.3e" % (k, d1, d0, bound))
    print("largest split / fp32 distance ratio: %.2f" % worst)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_deterministic_mode_same_bits_under_both_words(lib, use_graph):
    cfg, sd, batches, eps = _setup()
    lib.sln_set_deterministic(1)
    off = _run(lib, F32, cfg, sd, batches, eps, use_graph)
    on = _run(lib, SPLIT, cfg, sd, batches, eps, use_graph)
    for i, ((l1, g1), (l0, g0)) in enumerate(zip(on["steps"], off["steps"])):
        assert np.array_equal(l1, l0), "step %d: losses" % i
        for k in g0:
            assert np.array_equal(g1[k], g0[k], equal_nan=True), "step %d: gradient of %s differs between the words" % (i, k)
    LL._same_buffers(on, off, "split word, deterministic")


def test_a_word_change_between_replays_recaptures(lib):
    cfg, sd, batches, eps = _setup((3,))
    lib.sln_set_deterministic(0)
    m = LL._model(cfg, sd).train()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        captures, prev = 0, None
        for i, word in enumerate((F32, F32, SPLIT, SPLIT, F32)):
            assert lib.sln_set_tn_split(word) == 0
            m.train_step(*batches[0], kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=False)
            s.synchronize()
            assert lib.sln_get_tn_split() == word
            captures += 1 if word != prev else 0
            got = int(lib.sln_debug_vae_graph_captures(m._eng))
            assert got == captures, "step %d under word %d (before: %s): %d captures so far, expected %d" % (i, word, prev, got, captures)
            prev = word
        assert captures == 3


@pytest.mark.parametrize("name,ref,env", [("per-kind", {}, dict(SLN_TN_MIXED="0")), ("leaf-apart", {}, dict(SLN_TN_MIXED="1")),
                                          ("decoder-assembly-in-chain", {}, dict(SLN_TN_MIXED="2")),
                                          ("no-merge", dict(SLN_NO_MERGE="1", SLN_TN_MIXED="0"), dict(SLN_NO_MERGE="1"))])
def test_fallback_routes_equal_the_tail_launch_under_the_split(lib, name, ref, env):
    """The pairs of tests/test_vae_tail_launch_gpu.py: the tail launch against SLN_TN_MIXED=0 / 1 / 2, and SLN_NO_MERGE=1 (which
    restores older sum orders elsewhere in the step too) against itself with SLN_TN_MIXED=0, all under word 1."""
    cfg, sd, batches, eps = _setup()
    lib.sln_set_deterministic(0)
    t1 = _run(lib, SPLIT, cfg, sd, batches, eps, True, env=ref)
    t2 = _run(lib, SPLIT, cfg, sd, batches, eps, True, env=ref)
    fb = _run(lib, SPLIT, cfg, sd, batches, eps, True, env=env)
    noise = LL._noise(t1, t2)
    print("%s: spread of two tail-launch runs %.3e, fall-back against tail launch %.3e" % (name, noise, LL._noise(fb, t1)))
    LL._same_gradients(fb, t1, noise, name, exact=set(fb["bn"]))
    LL._same_buffers(fb, t1, name)


def test_three_adam_steps_in_lockstep(lib):
    """The protocol and bounds of tests/test_vae_leaf_launch_gpu.py::test_three_adam_steps_merged_against_unmerged, with the split
    word in the place of the merged build: two fp32-word models give the route's own run-to-run spread, and from equal states the
    split-word model's gradients, moments and parameters stay within 4 x that spread plus 4 ulp (parameters: 6) of the tensor's largest
    entry; tensors whose whole gradient is rounding residue move by Adam's own 2 lr at most.
    One exemption, per ELEMENT: a parameter element is held to that bound where its gradient is well away from zero - at least 1 %
    of its tensor's largest entry and at least 1e-5 (1 000 x Adam's eps) - and to 2 lr elsewhere.  Adam's update
    lr m / (sqrt(v) + 1e-8) is lr g / (|g| + 1e-8) in the first step: where |g| is a few 1e-8, a gradient difference of 1e-10 (the
    split's sums differ from the fp32 ones by real roundings, 2e-7 of a tensor's largest entry, in EVERY weight gradient, while the
    two fp32 models differ only where float atomics meet) becomes 1e-6 in the parameter, and a sign flip 2 lr.  For a held element
    dg <= 1.6e-6 max|g| <= 1.6e-4 |g| (the gradient bound above), so the first update moves by lr 1e-8 dg / g^2 <= 1.6e-10 and a later
    one by about lr dg / |g| <= 1.6e-7 lr: far inside the bound.  The number of held elements is printed."""
    cfg, sd, batches, eps = _setup((3, 4, 5))
    lib.sln_set_deterministic(0)
    models = {"u1": (F32, LL._model(cfg, sd).train()), "u2": (F32, LL._model(cfg, sd).train()), "sp": (SPLIT, LL._model(cfg, sd).train())}
    s = torch.cuda.Stream()
    bad = []
    with torch.cuda.stream(s):
        for i, b in enumerate(batches):
            st, losses = {}, {}
            first = models["u1"][1]
            for name, (_, m) in models.items():
                if i > 0 and name != "u1":                      # lockstep: every step starts from the first model's state
                    m.load_state_dict(first.state_dict())
                    m._adam_m.copy_(first._adam_m); m._adam_v.copy_(first._adam_v)
                    assert torch.equal(m.flat_params, first.flat_params)
                s.synchronize()
            for name, (word, m) in models.items():
                assert lib.sln_set_tn_split(word) == 0
                l = m.train_step(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=True)
                s.synchronize()
                st[name], losses[name] = LL._state(m), l.cpu().numpy().copy()
            assert np.array_equal(losses["sp"], losses["u1"]), "step %d: same parameters, same forward" % i
            gmax = max(float(np.abs(v).max()) for v in st["u1"]["grads"].values())
            residue = {k for k, v in st["u1"]["grads"].items() if float(np.abs(v).max()) < 1e-6 * gmax}
            for q in ("grads", "adam_m", "adam_v", "params"):
                a, b2, g = st["u1"][q], st["u2"][q], st["sp"][q]
                floor = 1e-6 * max(float(np.abs(v).max()) for v in a.values())
                scale = {k: max(float(np.abs(v).max()), floor) for k, v in a.items()}
                keys = [k for k in a if not (q == "params" and k in residue)]
                # parameters: the elements whose gradient is well away from zero (docstring); every element of the other quantities
                gr = st["u1"]["grads"]
                held = {k: ((np.abs(gr[k]) >= 1e-2 * float(np.abs(gr[k]).max())) & (np.abs(gr[k]) >= 1e-5)) if q == "params"
                        else np.ones(a[k].shape, bool) for k in a}
                dmax = lambda x, y, m: float(np.abs(x - y)[m].max()) if m.any() else 0.0
                spread = max(dmax(a[k], b2[k], held[k]) / scale[k] for k in keys)
                worst = max(dmax(g[k], a[k], held[k]) / scale[k] for k in keys)
                print("step %d %-7s fp32 run-to-run %.3e, split vs fp32 %.3e (%d of %d elements held)" % (
                    i, q, spread, worst, sum(int(held[k].sum()) for k in keys), sum(a[k].size for k in a)))
                for k in a:
                    if q == "params":
                        rest = np.ones(a[k].shape, bool) if k in residue else ~held[k]
                        d2 = dmax(g[k], a[k], rest)
                        if d2 > 2.02 * LR:
                            bad.append("step %d params %s: an exempt element differs by %.3e (2 lr)" % (i, k, d2))
                        if k in residue:
                            continue
                    d = dmax(g[k], a[k], held[k])
                    bound = (4.0 * spread + 4.0 * ULP + (2.0 * ULP if q == "params" else 0.0)) * scale[k]
                    if d > bound:
                        bad.append("step %d %s %s: differs by %.3e (bound %.3e)" % (i, q, k, d, bound))
    assert not bad, "\n".join(bad[:30])
