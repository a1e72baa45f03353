"""The leaf launch of a full VAE training iteration and W^T in the prologue (run with -m gpu on an MI355X).

A full iteration defers what nothing reads before the optimizer - three embedding-table gradients, the encoder's assembly
tables, the box embedding's Linear, the BatchNorm parameter gradients and the running statistics - to ONE launch at the end of
the backward pass, and rebuilds the transposed weights in its first launch.  `SLN_LEAF_MERGE=0` (read when the engine is
created) restores the per-kernel sequence; the test hook `sln_debug_vae_leaf_launches` tells which of the two an engine issued.

Bounds: the per-job arithmetic is the stand-alone kernels' own, so whatever carries no float atomics (losses, BatchNorm
running statistics and parameter gradients) must agree bit for bit; the other gradients within 4 x the spread that two runs of
the per-kernel sequence show against each other on the same inputs, plus 4 ulp where sums are unordered (see `_same_gradients`;
equality in deterministic mode).  Against the fp64 oracle
the project's 1e-4 criterion (tests/parity.py) holds, on a state without a ReLU or L1 threshold nearby.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from conftest import pkg
from parity import assert_close

pytestmark = pytest.mark.gpu

from oracle import vae_ref                                   # noqa: E402

BASE = dict(embedding_dim=32, gconv_num_layers=2)
LR = 1e-3


def _lib():
    return pkg("_lib")


@contextlib.contextmanager
def _environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(cfg, sd):
    M = pkg("host.Sg2ScVAE_model")
    m = M.Sg2ScVAEModel(**cfg.model_kwargs())
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.cuda()


def _batches(cfg, seeds, n_graphs=4, objs=8, triples=12):
    return [[t.cuda() for t in vae_ref.synth_batch(n_graphs, objs, triples, seed=s, cfg=cfg)[:5]] for s in seeds]


def _eps(cfg, rows, seed=0):
    return torch.randn(rows, cfg.embedding_dim, generator=torch.Generator().manual_seed(seed)).cuda()


def _bn_param_names(m):
    return [n + "." + w for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm1d) for w in ("weight", "bias")]


def _leaf_count(m):
    return int(_lib().lib().sln_debug_vae_leaf_launches(m._eng))


def _run(cfg, sd, batches, eps, merged, use_graph=False, with_adam=False, after=None):
    """One model, one train_step per batch.  Per step: (losses, {name: gradient}); at the end the BatchNorm buffers, the
    parameters and the engine's leaf-launch count.  `after(model)`: extra work behind the steps whose result is returned too."""
    with _environ(SLN_LEAF_MERGE=None if merged else "0"):          # read by sln_vae_create, at the first step
        m = _model(cfg, sd).train()
        s = torch.cuda.Stream()
        steps = []
        with torch.cuda.stream(s):
            for b in batches:
                l = m.train_step(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=use_graph, with_adam=with_adam)
                s.synchronize()
                steps.append((l.cpu().numpy().copy(), {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}))
            extra = after(m) if after is not None else None
            s.synchronize()
        bufs = {k: v.cpu().numpy().copy() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
        return dict(steps=steps, bufs=bufs, params=m.flat_params.cpu().numpy().copy(), leaf=_leaf_count(m), bn=_bn_param_names(m),
                    extra=extra)


def _noise(a, b):
    """The largest difference of two runs' gradients, relative to each tensor's own largest entry."""
    rel = 0.0
    for (_, ga), (_, gb) in zip(a["steps"], b["steps"]):
        for k in ga:
            scale = float(np.abs(ga[k]).max())
            if scale > 0.0 and np.isfinite(scale):
                rel = max(rel, float(np.nanmax(np.abs(ga[k] - gb[k]))) / scale)
    return rel


ULP = 2.0 ** -23


def _same_gradients(got, ref, noise, what, exact=(), ordered=False):
    """Every gradient of every step within 4 x `noise` + 4 ulp, both relative to the tensor's largest entry; the tensors named
    in `exact` and the losses bit for bit.  `ordered` (deterministic mode: every sum has one order): no ulp term, so a `noise`
    of 0 asks for equality.
    The ulp term: `noise` is what ONE pair of runs shows, and float atomics that happen to arrive in the same order twice give 0
    without the sums being ordered - seen on the batch without triples, where two runs of the per-kernel sequence agreed bit for
    bit and a third run of the SAME launch sequence (that case falls back to it) was 1.9e-9 / 3.7e-9 off in one table whose
    largest entry is 9.0e-2, in two of three repeats.  A sum taken in another order differs by roundings of its partial sums; 4 ulp
    of the largest entry is 5e-7 of it, the size of `noise` itself where it is not 0 (1.5e-7 - 2.8e-7 measured)."""
    bad = []
    for i, ((lg, gg), (lr_, gr)) in enumerate(zip(got["steps"], ref["steps"])):
        if not np.array_equal(lg, lr_):
            bad.append("%s step %d: losses %s vs %s" % (what, i, lg, lr_))
        for k in gr:
            if not np.array_equal(np.isnan(gg[k]), np.isnan(gr[k])):
                bad.append("%s step %d %s: NaN in other places" % (what, i, k))
                continue
            fin = ~np.isnan(gr[k])                 # (a batch without triples: BatchNorm over zero rows is NaN in both)
            d = float(np.abs(gg[k][fin] - gr[k][fin]).max()) if fin.any() else 0.0
            bound = 0.0 if k in exact or not fin.any() else (4.0 * noise + (0.0 if ordered else 4.0 * ULP)) * float(np.abs(gr[k][fin]).max())
            if d > bound:
                bad.append("%s step %d %s: differs by %.3e (bound %.3e, scale %.3e)" % (what, i, k, d, bound, float(np.abs(gr[k]).max())))
    assert not bad, "\n".join(bad[:30])


def _same_buffers(got, ref, what):
    for k in ref["bufs"]:
        a, b = got["bufs"][k], ref["bufs"][k]
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), "%s: %s" % (what, k)


# ------------------------------------------------------------------------------------------- Test 1: merged against unmerged
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_leaf_launch_gives_the_per_kernel_step(use_graph):
    """Two steps on two batches of one shape, eager and replayed: losses, BatchNorm buffers and BatchNorm parameter gradients
    bit for bit, every other gradient within 4 x the run-to-run spread of the per-kernel sequence."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = _batches(cfg, (3, 4))
    eps = _eps(cfg, batches[0][0].shape[0])
    u1 = _run(cfg, sd, batches, eps, merged=False, use_graph=use_graph)
    u2 = _run(cfg, sd, batches, eps, merged=False, use_graph=use_graph)
    mg = _run(cfg, sd, batches, eps, merged=True, use_graph=use_graph)
    noise = _noise(u1, u2)
    print("run-to-run spread of the per-kernel sequence: %.3e; merged vs per-kernel: %.3e" % (noise, _noise(mg, u1)))
    assert u1["leaf"] == 0 and u2["leaf"] == 0, "SLN_LEAF_MERGE=0 must keep the per-kernel sequence"
    assert mg["leaf"] == (1 if use_graph else 2), "one leaf launch per issued (or captured) iteration"
    _same_gradients(mg, u1, noise, "merged", exact=set(mg["bn"]))
    _same_buffers(mg, u1, "merged")


# ------------------------------------------------------------------------------------------- Tests 2 and 3: fp64 restatement
def _threshold_free(cfg, seed):
    """Train-mode BatchNorm state without a ReLU threshold nearby (see test_vae_gpu._threshold_free_state: the +8 sits on the
    BatchNorm beta, gamma in [0.5, 1]); fp32 and fp64 evaluations of such a step agree to ~1e-6."""
    sd = vae_ref.init_state(cfg, seed=seed, scale=0.1)
    for k, v in sd.items():
        mod = k.rsplit(".", 2)[-2] if k.count(".") >= 2 else ""
        if mod in ("1", "4") and v.dim() == 1 and k.endswith(".bias"):
            v.fill_(8.0)
        elif mod in ("1", "4") and v.dim() == 1 and k.endswith(".weight"):
            v.copy_(0.5 + (v - 0.5) * 0.5)
    return sd


def _fp64_step(cfg, sd, batch, eps):
    """(fp64 gradients, the batch with its L1 residuals moved away from 0, as the device takes it)."""
    batch = [t.clone() for t in batch]
    sg = torch.from_numpy(np.random.default_rng(7).integers(0, 2, tuple(batch[2].shape)).astype(np.float32)) * 2 - 1
    batch[2] = batch[2] + 20.0 * sg                         # per-element sign: one sign would vanish under the BatchNorm backward
    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    b64 = (batch[0], batch[1], batch[2].double(), batch[3], batch[4])
    keys = vae_ref.trainable_keys(cfg)
    m64 = {k: torch.zeros_like(sd64[k]) for k in keys}; v64 = {k: torch.zeros_like(sd64[k]) for k in keys}
    _, _, g64 = vae_ref.train_step(sd64, cfg, b64, eps.double(), 0.1, m64, v64, step=1, training=True)
    return g64, batch


def _leaf_keys(m):
    emb = [k for k, _ in m.named_parameters() if "embedding" in k]
    return emb + _bn_param_names(m)


def _against_fp64(got, g64, keys, what):
    bad = []
    for k in keys:
        ref = g64[k].numpy() if k in g64 else np.zeros(got[k].shape)
        atol = 1e-7 * max(float(np.abs(ref).max()), 1e-30) + 1e-9
        if k.endswith(".bias") and (k[:-len("bias")] + "weight") in g64 and float(np.abs(ref).max()) < 1e-12:
            # a BatchNorm beta whose exact gradient is 0 (a constant shift in front of another Linear -> BatchNorm): any fp32
            # evaluation returns the rounding residue of the cancelling sum, held to 1e-4 of the same module's gamma gradient
            atol = 1e-4 * float(np.abs(g64[k[:-len("bias")] + "weight"].numpy()).max())
        d = float(np.abs(got[k] - ref).max())
        print("%s %-50s err %.3e scale %.3e" % (what, k, d, float(np.abs(ref).max())))
        try:
            assert_close(got[k], ref, what + " grad:" + k, rtol=1e-4, atol=atol)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


def test_leaf_gradients_against_fp64():
    """The embedding tables (object, predicate and attribute ones of both nets, the angle one), the box embedding's Linear and every BatchNorm weight / bias of a merged step at 1e-4 of the fp64
    oracle: a deferred job that read an overwritten buffer is O(1) wrong."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = _threshold_free(cfg, seed=3)
    cpu = list(vae_ref.synth_batch(4, 8, 12, seed=0, cfg=cfg)[:5])
    eps = torch.from_numpy(np.random.default_rng(1).standard_normal((cpu[0].shape[0], cfg.embedding_dim)).astype(np.float32))
    g64, cpu = _fp64_step(cfg, sd, cpu, eps)
    run = _run(cfg, sd, [[t.cuda() for t in cpu]], eps.cuda(), merged=True)
    assert run["leaf"] == 1
    keys = [k for k in run["steps"][0][1] if "embedding" in k] + run["bn"]
    assert sum("embedding" in k for k in keys) == 9 and len(run["bn"]) > 0, keys       # seven tables + box_embeddings.weight / .bias
    _against_fp64(run["steps"][0][1], g64, keys, "merged")


def test_deferred_operands_survive_three_layers():
    """Three layers: the encoder's backward pass reuses both dG slots after the decoder's layer 0 wrote the operand of the
    deferred predicate-table job.  One predicate id occurs in exactly one triple, so its row of the decoder's (and the
    encoder's) predicate-table gradient is that triple's gradient row alone: checked against fp64, with both whole tables."""
    cfg = vae_ref.VaeConfig(embedding_dim=32, gconv_num_layers=3)
    sd = _threshold_free(cfg, seed=5)
    cpu = list(vae_ref.synth_batch(4, 8, 12, seed=2, cfg=cfg)[:5])
    tri = cpu[1].clone()
    lone = cfg.num_preds - 1
    tri[tri[:, 1] == lone, 1] = lone - 1
    first_random = int(torch.nonzero(tri[:, 1] != 0)[0])
    tri[first_random, 1] = lone
    assert int((tri[:, 1] == lone).sum()) == 1
    cpu[1] = tri
    eps = torch.from_numpy(np.random.default_rng(4).standard_normal((cpu[0].shape[0], cfg.embedding_dim)).astype(np.float32))
    g64, cpu = _fp64_step(cfg, sd, cpu, eps)
    run = _run(cfg, sd, [[t.cuda() for t in cpu]], eps.cuda(), merged=True)
    assert run["leaf"] == 1
    got = run["steps"][0][1]
    pred = [k for k in got if "pred_embeddings" in k]
    assert len(pred) == 2, pred
    for k in pred:
        ref = g64[k].numpy()
        assert float(np.abs(ref[lone]).max()) > 0.0
        d = float(np.abs(got[k][lone] - ref[lone]).max())
        print("%s row %d: err %.3e scale %.3e" % (k, lone, d, float(np.abs(ref[lone]).max())))
        assert_close(got[k][lone], ref[lone], k + " row of the lone predicate", rtol=1e-4, atol=1e-7 * float(np.abs(ref[lone]).max()) + 1e-9)
    _against_fp64(got, g64, pred, "three layers")


# ------------------------------------------------------------------------------------------- Test 4: fall-backs
def _fallback_case(name):
    kw = dict(BASE)
    det, empty_t = False, False
    if name == "deterministic":
        det = True
    elif name == "large_vocabulary":
        kw["num_objs"] = 512                       # 512 rows x 24 columns = 12 288 floats: past the 10 240-float LDS cap of the assembly tables
    elif name == "no_triples":
        empty_t = True
    elif name == "no_attributes":
        kw["use_attr"] = False
    elif name == "decoder_cat_off":
        kw["decoder_cat"] = False
    return vae_ref.VaeConfig(**kw), det, empty_t


@pytest.mark.parametrize("name", ["deterministic", "large_vocabulary", "no_triples", "no_attributes", "decoder_cat_off"])
def test_fallbacks_keep_the_per_kernel_sequence(name):
    """What the leaf launch does not take - deterministic mode, a vocabulary past the LDS cap, a batch without triples, a model
    without attribute embeddings or with z joining behind the decoder's gconv net - runs the per-kernel sequence: no leaf launch,
    the gradients of `SLN_LEAF_MERGE=0`.  Deterministic mode repeats bit for bit."""
    cfg, det, empty_t = _fallback_case(name)
    sd = vae_ref.init_state(cfg, seed=6)
    batches = _batches(cfg, (5,))
    if empty_t:
        batches[0][1] = batches[0][1][:0].contiguous()
    eps = _eps(cfg, batches[0][0].shape[0])
    L = _lib().lib()
    try:
        L.sln_set_deterministic(int(det))
        u1 = _run(cfg, sd, batches, eps, merged=False)
        u2 = _run(cfg, sd, batches, eps, merged=False)
        d1 = _run(cfg, sd, batches, eps, merged=True)
        d2 = _run(cfg, sd, batches, eps, merged=True) if det else None
    finally:
        L.sln_set_deterministic(0)
    noise = _noise(u1, u2)
    print("%s: run-to-run spread %.3e, default vs SLN_LEAF_MERGE=0 %.3e" % (name, noise, _noise(d1, u1)))
    assert d1["leaf"] == 0 and u1["leaf"] == 0, "the leaf launch must not be used"
    _same_gradients(d1, u1, noise, name, exact=set(d1["bn"]), ordered=det)
    _same_buffers(d1, u1, name)
    if det:
        assert noise == 0.0, "deterministic mode: two runs of the per-kernel sequence differ"
        _same_gradients(d2, d1, 0.0, "deterministic, second run", ordered=True)
        _same_buffers(d2, d1, "deterministic, second run")


# ------------------------------------------------------------------------------------------- Test 5: W^T
def test_no_stale_transposes_after_new_parameters():
    """A step, then load_state_dict of other parameters (which tells the engine), then a replayed step: the gradients of a fresh
    model with those parameters.  A W^T left over from the first parameters would be O(1) off."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd_a, sd_b = vae_ref.init_state(cfg, seed=8), vae_ref.init_state(cfg, seed=9)
    batches = _batches(cfg, (3,))
    eps = _eps(cfg, batches[0][0].shape[0])

    def fresh(merged):
        return _run(cfg, sd_b, batches, eps, merged=merged, use_graph=True)

    def reloaded():
        def second(m):
            m.load_state_dict({k: v.clone() for k, v in sd_b.items()})
            l = m.train_step(*batches[0], kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=False)
            torch.cuda.current_stream().synchronize()
            return dict(steps=[(l.cpu().numpy().copy(), {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()})])
        return _run(cfg, sd_a, batches, eps, merged=True, use_graph=True, after=second)["extra"]

    u1, u2 = fresh(False), fresh(False)
    noise = _noise(u1, u2)
    f = fresh(True)
    r = reloaded()
    print("spread %.3e, reloaded vs fresh %.3e" % (noise, _noise(r, f)))
    _same_gradients(r, f, noise, "reloaded", exact=set(f["bn"]))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_autograd_backward_after_a_fused_step(use_graph):
    """A stand-alone backward() through the autograd path behind a fused step (which leaves its transposed weights valid when
    it ran eagerly, and stale ones behind a replay) gives what the per-kernel build gives."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = _batches(cfg, (3,))
    eps = _eps(cfg, batches[0][0].shape[0])
    w = [torch.randn(batches[0][0].shape[0], n, generator=torch.Generator().manual_seed(i)).cuda()
         for i, n in enumerate((cfg.embedding_dim, cfg.embedding_dim, cfg.box_dim, cfg.Nangle))]

    def autograd(m):
        m.zero_grad()
        out = m(*batches[0], None, eps=eps)
        sum((o * wi).sum() for o, wi in zip(out, w)).backward()
        torch.cuda.current_stream().synchronize()
        return dict(steps=[(np.zeros(1), {k: (p.grad.detach().cpu().numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                                          for k, p in m.named_parameters()})])

    u1 = _run(cfg, sd, batches, eps, merged=False, use_graph=use_graph, after=autograd)
    u2 = _run(cfg, sd, batches, eps, merged=False, use_graph=use_graph, after=autograd)
    mg = _run(cfg, sd, batches, eps, merged=True, use_graph=use_graph, after=autograd)
    noise = _noise(u1["extra"], u2["extra"])
    print("spread %.3e, merged vs per-kernel %.3e" % (noise, _noise(mg["extra"], u1["extra"])))
    assert mg["leaf"] == 1, "the stand-alone backward keeps its own launches"
    _same_gradients(mg["extra"], u1["extra"], noise, "autograd backward", exact=set(mg["bn"]))


# ------------------------------------------------------------------------------------------- Test 6: with Adam
def _state(m):
    """What a step with the optimizer leaves, cut into tensors: {quantity: {name: array}}."""
    g0 = m.flat_grads.data_ptr()
    spans = {k: ((p.grad.data_ptr() - g0) // 4, p.numel()) for k, p in m.named_parameters()}        # a tensor's place in the flat buffers
    flat = dict(grads=m.flat_grads, adam_m=m._adam_m, adam_v=m._adam_v, params=m.flat_params)
    flat = {q: v.cpu().numpy().copy() for q, v in flat.items()}
    return {q: {k: v[o:o + n] for k, (o, n) in spans.items()} for q, v in flat.items()}


def test_three_adam_steps_merged_against_unmerged():
    """Three replayed steps with the optimizer: the merged build against `SLN_LEAF_MERGE=0`, and a second `SLN_LEAF_MERGE=0`
    model as the yardstick of the per-kernel sequence's own noise.

    The noise bound of the first test is propagated step by step: the three models run in lockstep, and before steps 2 and 3
    the two others take over the first model's parameters, BatchNorm buffers and Adam moments.  Left to run free, the trajectories
    part on their own, the two per-kernel ones among themselves just as the merged one from them: of three trials on an MI355X,
    two had ~90 of the tensors differ after the third step between the two PER-KERNEL runs (gradients 1.6e-6 / 8.8e-6 apart instead
    of 1.6e-7; the merged run against them: 1.8e-6 / 8.5e-6) and one had none.  An element of a parameter crosses a rounding
    boundary in one run's update and not in the other's, and every Linear bias in front of a train-mode BatchNorm, whose exact
    gradient is 0, moves by +-lr with the sign of its rounding residue.  A spread measured on one pair of free runs is therefore
    either ~2e-7 or ten times that, and says nothing about the next pair.

    From equal states, after every step and for every tensor:
      * the gradients and Adam's moments (linear and quadratic in the gradients: a leaf job that read a wrong buffer is O(1) off
        there) within 4 x the spread of the two per-kernel models in the same quantity of the same step plus 4 ulp (as
        `_same_gradients`), relative to the tensor's largest entry, and to no less than 1e-6 of the largest entry of all for tensors that hold only rounding residue;
      * the parameters within that and 2 ulp of the tensor's largest entry (the same update from gradients 1e-7 apart lands
        on the next fp32 neighbour at most); tensors whose whole gradient is residue (below 1e-6 of the step's largest gradient
        entry) within Adam's own 2 lr, the sign of a residue being arbitrary."""
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = _batches(cfg, (3, 4, 5))
    eps = _eps(cfg, batches[0][0].shape[0])
    models = {}
    for name, merged in (("u1", False), ("u2", False), ("mg", True)):
        models[name] = _model(cfg, sd).train()
    s = torch.cuda.Stream()
    bad = []
    with torch.cuda.stream(s):
        for i, b in enumerate(batches):
            st, losses = {}, {}
            for name, m in models.items():
                if i > 0 and name != "u1":                      # lockstep: every step starts from the first model's state
                    m.load_state_dict(models["u1"].state_dict())
                    m._adam_m.copy_(models["u1"]._adam_m); m._adam_v.copy_(models["u1"]._adam_v)
                    assert torch.equal(m.flat_params, models["u1"].flat_params)
                s.synchronize()
            for name, m in models.items():
                with _environ(SLN_LEAF_MERGE=None if name == "mg" else "0"):          # read when the first step creates the engine
                    l = m.train_step(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=True)
                s.synchronize()
                st[name], losses[name] = _state(m), l.cpu().numpy().copy()
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
                print("step %d %-7s per-kernel run-to-run %.3e, merged vs per-kernel %.3e" % (i, q, spread, worst))
                for k in a:
                    d = float(np.abs(g[k] - a[k]).max())
                    if q == "params" and k in residue:
                        bound = 2.02 * LR
                    else:
                        bound = (4.0 * spread + 4.0 * ULP + (2.0 * ULP if q == "params" else 0.0)) * scale[k]
                    if d > bound:
                        bad.append("step %d %s %s: differs by %.3e (bound %.3e)" % (i, q, k, d, bound))
    assert _leaf_count(models["mg"]) == 1 and _leaf_count(models["u1"]) == 0 and _leaf_count(models["u2"]) == 0
    assert not bad, "\n".join(bad[:30])
