"""Time the layout evaluation (reference testing/test_acc_mean_std.py: get_acc_l1 + get_std, test.py --measure_acc_l1_std) on the
GPU box: measure_acc_l1_std on synthetic batches of 64 graphs with a small and the BASELINE-size model, the metric launches alone
(baselines + relation S=3 + L1 + spread of one batch), and the torch restatement of the same metric work on the CPU (16 threads)."""
import os
import sys
import time
import importlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

M = importlib.import_module("3d_sln_amd.host.Sg2ScVAE_model"); syn = importlib.import_module("3d_sln_amd.host.synthetic")
E = importlib.import_module("3d_sln_amd.host.evaluate")

N_BATCHES, GRAPHS, OBJS, TRIPLES = 8, 64, 10, 20
vocab = dict(syn.default_vocab(), pred_idx_to_name=list(E.RELATIONSHIPS))
batches = []
for i in range(N_BATCHES):
    b = syn.scene_graph_batch(GRAPHS, OBJS, TRIPLES, seed=i, device="cuda")
    batches.append((b["objs"], b["triples"], b["boxes"], b["angles"], b["attributes"]))
O, T = batches[0][0].shape[0], batches[0][1].shape[0]
print("%d batches of %d graphs: O = %d rows, T = %d triples per batch" % (N_BATCHES, GRAPHS, O, T))


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


for tag, E_dim, layers in (("small (E=16, 2 layers)", 16, 2), ("BASELINE (E=64, 5 layers)", 64, 5)):
    torch.manual_seed(0)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=E_dim, gconv_mode='feedforward',
                            gconv_num_layers=layers, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    mean = torch.zeros(E_dim, dtype=torch.float64); cov = torch.eye(E_dim, dtype=torch.float64)
    dt = timed(lambda: E.measure_acc_l1_std(model, batches, mean, cov, vocab, seed=1), 5)
    print("measure_acc_l1_std, %s: %.2f ms for %d batches (%.3f ms per 64-graph batch)" % (tag, dt * 1e3, N_BATCHES, dt * 1e3 / N_BATCHES))

# the metric launches alone, one batch
objs, triples, boxes, angles, attrs = batches[0]
room, tab = E.room_class(vocab), E.relation_table(vocab)
lay = torch.empty(3, O, 6, device="cuda"); lay[0] = boxes + 0.01
dec = boxes[None].repeat(10, 1, 1) + 0.01 * torch.randn(10, O, 6, device="cuda")
bins = torch.randint(0, 24, (10, O), device="cuda")
key = torch.zeros(2, dtype=torch.int64, device="cuda")
good = torch.zeros(3, dtype=torch.int64, device="cuda"); l1 = torch.zeros(3, dtype=torch.float64, device="cuda")
sp = torch.zeros(3, dtype=torch.float64, device="cuda")
parts = {"baselines": lambda: E.baselines(boxes, objs, room, key=key, out=lay[1:]),
         "relation (S=3)": lambda: E.relation_acc(lay, objs, triples, room, tab, good=good),
         "l1 (S=3)": lambda: E.layout_l1(lay, boxes, out=l1),
         "spread (10 samples)": lambda: E.layout_spread(dec, bins, out=sp)}
tot = 0.0
for name, fn in parts.items():
    dt = timed(fn, 200)
    tot += dt
    print("  %-20s %7.1f us" % (name, dt * 1e6))
print("  metric launches per batch: %.1f us (host wall clock per launch, back to back)" % (tot * 1e6))

# CPU: the torch restatement of the same metric work, 16 threads
torch.set_num_threads(16)
c = [t.cpu() for t in (objs, triples, boxes, lay, dec, bins)]
u = torch.rand(O, 3); n = torch.randn(O, 3) * 0.1


def cpu_metrics():
    bl = E.baselines_torch(c[2], c[0], room, u, n)
    lays = torch.cat([c[3][:1], bl])
    E.relation_acc_torch(lays, c[0], c[1], room, tab)
    E.layout_l1_torch(lays, c[2])
    E.layout_spread_torch(c[4], c[5])


t0 = time.perf_counter()
for _ in range(20):
    cpu_metrics()
dt = (time.perf_counter() - t0) / 20
print("CPU torch restatement of the metric work (16 threads): %.2f ms per 64-graph batch" % (dt * 1e3))
