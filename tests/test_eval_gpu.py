"""Layout evaluation on the device (host/evaluate.py: sln_layout_relation_acc / _l1 / _spread / _baselines, measure_acc_l1_std)
against the reference's own get_acc_l1 / get_std / scene_graph_acc (tests/golden/eval_metrics.npz, tools/gen_golden_eval.py)."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, pkg

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _fixture():
    g = load_golden("eval_metrics")
    meta = json.loads(bytes(g["meta"]).decode())
    vocab = dict(object_idx_to_name=meta["object_idx_to_name"], pred_idx_to_name=meta["pred_idx_to_name"])
    return g, meta, vocab


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _batch(g, b):
    k = "b%d:" % b
    return (None, _d(g[k + "objs"]), _d(g[k + "boxes"]), _d(g[k + "triples"]), _d(g[k + "angles"]), _d(g[k + "attributes"]),
            _d(g[k + "obj_to_img"]), None)


def _draws(g, meta):
    return [dict(z=_d(g["b%d:z" % b]), uniforms=_d(g["b%d:uniforms" % b], torch.float32), normals=_d(g["b%d:normals" % b], torch.float32),
                 z_std=_d(g["b%d:z_std" % b])) for b in range(meta["n_batches"])]


def _model(meta):
    from oracle import vae_ref
    M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(**meta["cfg"])
    sd = vae_ref.init_state(cfg, seed=meta["weight_seed"])
    m = M.Sg2ScVAEModel(**cfg.model_kwargs())
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    return m.to(DEV).eval()


def test_relation_kernel_equals_the_reference_counts():
    """the reference's recorded layouts (predicted, random, perturbed: S = 3 in one launch) -> good, exactly, under both vocabularies"""
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    alt = dict(vocab, pred_idx_to_name=meta["alt_pred_idx_to_name"])
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        lay = _d(g[k + "layouts"])
        before = lay.clone()
        for voc, key in ((vocab, "good"), (alt, "good_alt")):
            good, _ = E.relation_acc(lay, _d(g[k + "objs"]), _d(g[k + "triples"]), E.room_class(voc), E.relation_table(voc))
            assert good.cpu().tolist() == g[k + key].tolist(), (b, key)
        assert torch.equal(lay, before)                             # the caller's tensor is not restored in place


@pytest.mark.parametrize("case", ["nan", "room_not_last", "after_last_room", "zero_area"])
def test_relation_kernel_hand_made_cases(case):
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    alt = dict(vocab, pred_idx_to_name=meta["alt_pred_idx_to_name"])
    objs, boxes, tr = _d(g["case:%s:objs" % case]), _d(g["case:%s:boxes" % case]), _d(g["case:%s:triples" % case])
    for vname, voc in (("vocab", vocab), ("alt", alt)):
        good, conf = E.relation_acc(boxes[None], objs, tr, E.room_class(voc), E.relation_table(voc), confusion=True)
        assert int(good[0]) == int(g["case:%s:%s:good" % (vname, case)]), vname
        want_g, want_c = E.relation_acc_torch(boxes[None].cpu(), objs.cpu(), tr.cpu(), E.room_class(voc), E.relation_table(voc))
        assert torch.equal(conf.cpu(), want_c), vname


def test_confusion_table_equals_the_cpu_restatement():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        lay, objs, tr = _d(g[k + "layouts"]), _d(g[k + "objs"]), _d(g[k + "triples"])
        good, conf = E.relation_acc(lay, objs, tr, E.room_class(vocab), E.relation_table(vocab), confusion=True)
        _, want = E.relation_acc_torch(lay.cpu(), objs.cpu(), tr.cpu(), E.room_class(vocab), E.relation_table(vocab))
        conf = conf.cpu()
        assert torch.equal(conf, want), b
        per_pred = torch.bincount(tr[:, 1].cpu(), minlength=16)
        for s in range(3):
            assert conf[s].sum(1).tolist() == per_pred.tolist()
        assert conf.diagonal(dim1=1, dim2=2).sum(1).tolist() == good.cpu().tolist()


def test_baselines_replay_the_reference_bit_for_bit():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        out = E.baselines(_d(g[k + "boxes"]), _d(g[k + "objs"]), E.room_class(vocab), uniforms=_d(g[k + "uniforms"], torch.float32),
                          normals=_d(g[k + "normals"], torch.float32))
        assert np.array_equal(out.cpu().numpy(), g[k + "layouts"][1:]), b


def test_l1_and_spread_from_the_reference_decodes():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        l1 = E.layout_l1(_d(g[k + "layouts"]), _d(g[k + "boxes"])).cpu().numpy()
        np.testing.assert_allclose(l1, g[k + "l1"], rtol=1e-6)
        sp = E.layout_spread(_d(g[k + "std_boxes"]), _d(g[k + "std_angles"])).cpu().numpy()
        np.testing.assert_allclose(sp, g[k + "std"], rtol=1e-5)
        sp2 = E.layout_spread(_d(g[k + "std_boxes"]), _d(g[k + "std_angles"])).cpu().numpy()
        assert np.array_equal(sp, sp2)                                # fixed-order reduction: bit-identical


def test_device_draws():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    k = "b2:"
    gt, objs = _d(g[k + "boxes"]), _d(g[k + "objs"])
    room = E.room_class(vocab)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    key = torch.randint(-2 ** 62, 2 ** 62, (2,), dtype=torch.int64, device=DEV, generator=gen)
    a = E.baselines(gt, objs, room, key=key).cpu()
    b = E.baselines(gt, objs, room, key=key).cpu()
    assert torch.equal(a, b)
    key2 = key.clone()
    key2[0] += 1
    c = E.baselines(gt, objs, room, key=key2).cpu()
    assert not torch.equal(a, c)
    gtc, is_room = gt.cpu(), (objs.cpu() == room)
    rnd, per = a[0], a[1]
    assert torch.equal(rnd[is_room], gtc[is_room])
    ctr = (rnd[~is_room, :3] + rnd[~is_room, 3:]) / 2
    assert float(ctr.min()) >= -1e-6 and float(ctr.max()) < 1.0 + 1e-6
    ext = gtc[~is_room, 3:] - gtc[~is_room, :3]
    assert torch.allclose(rnd[~is_room, 3:] - rnd[~is_room, :3], ext, atol=1e-6)
    off = per - gtc
    assert torch.allclose(off[:, :3], off[:, 3:], atol=1e-6)
    # spread of the offsets over a larger draw
    big = torch.rand(4096, 6, device=DEV)
    big[:, 3:] += big[:, :3]
    o = E.baselines(big, torch.ones(4096, dtype=torch.int64, device=DEV), room, key=key).cpu()
    d = (o[1] - big.cpu())[:, :3].double()
    assert abs(float(d.std()) - 0.1) < 0.006 and abs(float(d.mean())) < 0.006
    u = ((o[0][:, :3] + o[0][:, 3:]) / 2).double()
    assert abs(float(u.mean()) - 0.5) < 0.02 and float(u.min()) >= -1e-6 and float(u.max()) < 1.0 + 1e-6


def test_edge_cases():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    room, tab = E.room_class(vocab), E.relation_table(vocab)
    k = "b1:"
    lay, objs = _d(g[k + "layouts"]), _d(g[k + "objs"])
    good, conf = E.relation_acc(lay, objs, torch.zeros(0, 3, dtype=torch.int64, device=DEV), room, tab, confusion=True)
    assert good.cpu().tolist() == [0, 0, 0] and int(conf.sum()) == 0                  # T = 0
    sp = E.layout_spread(lay[:1], torch.zeros(1, lay.shape[1], dtype=torch.int64, device=DEV))
    assert sp.cpu().tolist() == [0.0, 0.0, 0.0]                                         # S = 1: std 0
    with pytest.raises(ValueError):
        E.relation_acc(torch.zeros(1, 3, 4, device=DEV), objs[:3], torch.zeros(1, 3, dtype=torch.int64, device=DEV), room, tab)
    with pytest.raises(ValueError):
        E.layout_spread(torch.zeros(2, 3, 4, device=DEV), torch.zeros(2, 3, dtype=torch.int64, device=DEV))
    L = pkg("_lib")
    with pytest.raises(L.SlnError):                                                     # the library itself refuses box_dim 4
        L.check(L.lib().sln_layout_l1(L.ptr(lay), 3, lay.shape[1], 4, L.ptr(lay[0]), L.ptr(torch.zeros(3, dtype=torch.float64, device=DEV)),
                                      L.current_stream_ptr()), "sln_layout_l1")


def test_measure_acc_l1_std_end_to_end():
    """the fixture's weights and injected draws: L1 and stds within 1e-4 of what the reference printed; relation accuracy within a
    few triples, in two steps: the device decodes are within 1e-4 of the reference's, and the device kernel on the device's own
    decodes equals the CPU restatement on those boxes exactly - any count difference is a threshold flip of the decode"""
    E = pkg("host.evaluate")
    S = pkg("host.sampling")
    g, meta, vocab = _fixture()
    model = _model(meta)
    batches = [_batch(g, b) for b in range(meta["n_batches"])]
    draws = _draws(g, meta)
    mean, cov = torch.from_numpy(g["mean"]), torch.from_numpy(g["cov"])
    res = E.measure_acc_l1_std(model, batches, mean, cov, vocab, n_std_samples=meta["nsample"], draws=draws)
    pr = g["printed"]
    got = [res[k] for k in ("l1_pred", "l1_rand", "l1_pert", "acc_pred", "acc_rand", "acc_pert", "angle_std", "position_std", "size_std")]
    for i in (0, 1, 2, 6, 7, 8):
        assert abs(got[i] - pr[i]) <= 1e-4 * max(1.0, abs(pr[i])), (i, got[i], pr[i])
    assert got[4] == pr[4] and got[5] == pr[5]                     # the baselines are replayed exactly
    room, tab = E.room_class(vocab), E.relation_table(vocab)
    flips, tot = 0, 0
    for b in range(meta["n_batches"]):
        _, objs, boxes, triples, _, attrs, _, _ = batches[b]
        bp, _, _ = S.sample_layouts(model, objs, triples, attrs, n_samples=1, z=draws[b]["z"])
        ref = torch.from_numpy(g["b%d:pred_boxes" % b])
        assert torch.allclose(bp[0].cpu(), ref, rtol=1e-4, atol=1e-4), b
        good, _ = E.relation_acc(bp.contiguous(), objs, triples, room, tab)
        want, _ = E.relation_acc_torch(bp.cpu(), objs.cpu(), triples.cpu(), room, tab)
        assert good.cpu().tolist() == want.tolist(), b
        flips += abs(int(good[0]) - int(g["b%d:good" % b][0]))
        tot += int(triples.shape[0])
    print("threshold flips of the device decodes: %d of %d triples" % (flips, tot))
    assert abs(got[3] - pr[3]) * tot <= max(3, flips) and flips <= 6


def test_measure_acc_l1_std_is_reproducible():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    model = _model(meta)
    batches = [_batch(g, b) for b in range(meta["n_batches"])]
    mean, cov = torch.from_numpy(g["mean"]), torch.from_numpy(g["cov"])
    a = E.measure_acc_l1_std(model, batches, mean, cov, vocab, seed=11)
    b = E.measure_acc_l1_std(model, batches, mean, cov, vocab, seed=11)
    c = E.measure_acc_l1_std(model, batches, mean, cov, vocab, seed=12)
    assert a == b
    assert a != c
    assert all(np.isfinite(v) for v in a.values()) and 0.0 <= a["acc_pred"] <= 1.0
    d = E.measure_acc_l1_std(model, batches[:1], mean, cov, vocab)         # the engine's own stream
    assert all(np.isfinite(v) for v in d.values())
