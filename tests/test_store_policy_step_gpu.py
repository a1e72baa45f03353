"""The VAE training step under the two store policies of the NT GEMM epilogues (sln_set_store_policy; run with -m gpu on an MI355X).

4 graphs x (8 objects, 12 triples), the helpers and bounds of tests/test_vae_leaf_launch_gpu.py.  The policy moves no value and no
sum order, so:
  * in deterministic mode (every sum has one order) losses, BatchNorm buffers and ALL gradients are equal bit for bit, write-through
    against plain, eager and replayed;
  * in default mode the wgrads add with float atomics in arrival order: gradients within 4 x the spread of two plain-store runs plus
    4 ulp of the tensor's largest entry (LL._same_gradients), losses / BatchNorm buffers / BatchNorm parameters bit for bit;
  * three Adam steps in lockstep, the leaf-launch test's protocol;
  * a policy change between two replays re-captures: the engine drops its captured iterations when the policy word differs from
    the one they were recorded under, as it does for deterministic mode.  Values cannot show which instantiation a replay ran, so
    the test reads the engine's capture counter (sln_debug_vae_graph_captures): it must go up by one exactly at each change of the
    word and stay between equal words."""
import numpy as np
import pytest
import torch

import test_vae_leaf_launch_gpu as LL
from oracle import vae_ref

pytestmark = pytest.mark.gpu

BASE, LR, ULP = LL.BASE, LL.LR, LL.ULP
PLAIN, NT_WT = 0, 1


@pytest.fixture
def lib():
    h = LL._lib().lib()
    pol, det = h.sln_get_store_policy(), h.sln_get_deterministic()
    yield h
    assert h.sln_set_store_policy(pol) == 0
    h.sln_set_deterministic(det)


def _run(h, policy, cfg, sd, batches, eps, use_graph, with_adam=False):
    assert h.sln_set_store_policy(policy) == 0
    return LL._run(cfg, sd, batches, eps, True, use_graph=use_graph, with_adam=with_adam)


def _setup(seeds=(3, 4)):
    cfg = vae_ref.VaeConfig(**BASE)
    sd = vae_ref.init_state(cfg, seed=8)
    batches = LL._batches(cfg, seeds)
    return cfg, sd, batches, LL._eps(cfg, batches[0][0].shape[0])


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_deterministic_mode_bit_for_bit(lib, use_graph):
    cfg, sd, batches, eps = _setup()
    lib.sln_set_deterministic(1)
    off = _run(lib, PLAIN, cfg, sd, batches, eps, use_graph)
    on = _run(lib, NT_WT, cfg, sd, batches, eps, use_graph)
    for i, ((l1, g1), (l0, g0)) in enumerate(zip(on["steps"], off["steps"])):
        assert np.array_equal(l1, l0), "step %d: losses %s vs %s" % (i, l1, l0)
        for k in g0:
            assert np.array_equal(g1[k], g0[k], equal_nan=True), "step %d: gradient of %s differs between the policies" % (i, k)
    LL._same_buffers(on, off, "write-through, deterministic")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_default_mode_within_the_plain_spread(lib, use_graph):
    cfg, sd, batches, eps = _setup()
    lib.sln_set_deterministic(0)
    u1 = _run(lib, PLAIN, cfg, sd, batches, eps, use_graph)
    u2 = _run(lib, PLAIN, cfg, sd, batches, eps, use_graph)
    on = _run(lib, NT_WT, cfg, sd, batches, eps, use_graph)
    noise = LL._noise(u1, u2)
    print("spread of two plain-store runs %.3e; write-through against plain %.3e" % (noise, LL._noise(on, u1)))
    LL._same_gradients(on, u1, noise, "write-through", exact=set(on["bn"]))
    LL._same_buffers(on, u1, "write-through")


def test_a_policy_change_between_replays_recaptures(lib):
    """One model, replayed steps on one batch: plain, plain, write-through, write-through, plain, plain, and a set of the SAME word
    between two replays.  A replay of the old graph would run the other policy's kernels with nothing to show for it in the values,
    so the engine's capture counter is held: +1 at the first step and at each change of the word, +0 otherwise.  In deterministic
    mode every step from the same state gives the same bits, so the steps must also agree among themselves."""
    cfg, sd, batches, eps = _setup((3,))
    lib.sln_set_deterministic(1)
    m = LL._model(cfg, sd).train()
    s = torch.cuda.Stream()
    out = []
    with torch.cuda.stream(s):
        seq = (PLAIN, PLAIN, NT_WT, NT_WT, NT_WT, PLAIN, PLAIN)
        captures, prev = 0, None
        for i, pol in enumerate(seq):
            assert lib.sln_set_store_policy(pol) == 0
            l = m.train_step(*batches[0], kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=False)
            s.synchronize()
            assert lib.sln_get_store_policy() == pol
            captures += 1 if pol != prev else 0
            got = int(lib.sln_debug_vae_graph_captures(m._eng))
            assert got == captures, "step %d under policy %d (before: %s): %d captures so far, expected %d" % (i, pol, prev, got, captures)
            prev = pol
            out.append((pol, l.cpu().numpy().copy(), m.flat_grads.cpu().numpy().copy()))
        assert captures == 3
    for pol, l, g in out[1:]:
        assert np.array_equal(l, out[0][1]) and np.array_equal(g, out[0][2], equal_nan=True), "policy %d: the replayed step changed" % pol


def test_three_adam_steps_in_lockstep(lib):
    """As tests/test_vae_leaf_launch_gpu.py::test_three_adam_steps_merged_against_unmerged, in deterministic mode: from equal states
    a step with the optimizer leaves the same gradients, moments and parameters under both policies, three times in a row."""
    cfg, sd, batches, eps = _setup((3, 4, 5))
    lib.sln_set_deterministic(1)
    models = {PLAIN: LL._model(cfg, sd).train(), NT_WT: LL._model(cfg, sd).train()}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i, b in enumerate(batches):
            st = {}
            if i > 0:                                           # lockstep: every step starts from the plain model's state
                m = models[NT_WT]
                m.load_state_dict(models[PLAIN].state_dict())
                m._adam_m.copy_(models[PLAIN]._adam_m); m._adam_v.copy_(models[PLAIN]._adam_v)
                assert torch.equal(m.flat_params, models[PLAIN].flat_params)
                s.synchronize()
            for pol, m in models.items():
                assert lib.sln_set_store_policy(pol) == 0
                l = m.train_step(*b, kl_weight=0.1, lr=LR, eps=eps, use_graph=True, with_adam=True)
                s.synchronize()
                st[pol] = (l.cpu().numpy().copy(), LL._state(m))
            assert np.array_equal(st[NT_WT][0], st[PLAIN][0]), "step %d: losses" % i
            for q, tensors in st[PLAIN][1].items():
                for k, v in tensors.items():
                    assert np.array_equal(st[NT_WT][1][q][k], v, equal_nan=True), "step %d: %s of %s differs between the policies" % (i, q, k)
