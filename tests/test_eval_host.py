"""Torch restatements of the layout-evaluation kernels (host/evaluate.py) against the reference's own get_acc_l1 / get_std /
scene_graph_acc, executed from their source by tools/gen_golden_eval.py (tests/golden/eval_metrics.npz).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, pkg


def _fixture():
    g = load_golden("eval_metrics")
    meta = json.loads(bytes(g["meta"]).decode())
    vocab = dict(object_idx_to_name=meta["object_idx_to_name"], pred_idx_to_name=meta["pred_idx_to_name"])
    return g, meta, vocab


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_relation_table_and_room_class():
    E = pkg("host.evaluate")
    _, meta, vocab = _fixture()
    assert E.relation_table(vocab).tolist() == list(range(16))
    alt = dict(vocab, pred_idx_to_name=meta["alt_pred_idx_to_name"])
    tab = E.relation_table(alt).tolist()
    for r, name in enumerate(E.RELATIONSHIPS):
        assert tab[r] == (meta["alt_pred_idx_to_name"].index(name) if name in meta["alt_pred_idx_to_name"] else -1)
    assert sum(t < 0 for t in tab) == 3
    syn = pkg("host.synthetic").default_vocab()                  # predicates named pred00..: nothing can match
    assert E.relation_table(syn).tolist() == [-1] * 16
    assert E.room_class(dict(object_idx_to_name=["a", "b", "__room__"])) == 2
    with pytest.raises(ValueError):
        E.relation_table(dict(pred_idx_to_name=["on", "on"]))


def test_relation_acc_torch_reproduces_the_reference_counts():
    """good counts of the predicted / random / perturbed layouts of every batch, under the reference vocabulary and under one that
    lacks three relation names and orders the rest differently"""
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    alt = dict(vocab, pred_idx_to_name=meta["alt_pred_idx_to_name"])
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        objs, tr, lay = _t(g[k + "objs"]), _t(g[k + "triples"]), _t(g[k + "layouts"])
        before = lay.clone()
        for voc, key in ((vocab, "good"), (alt, "good_alt")):
            good, conf = E.relation_acc_torch(lay, objs, tr, E.room_class(voc), E.relation_table(voc))
            assert good.tolist() == g[k + key].tolist(), (b, key)
            assert conf.diagonal(dim1=1, dim2=2).sum(1).tolist() == good.tolist()
        assert torch.equal(lay, before)                               # restore_box is applied out of place


@pytest.mark.parametrize("case", ["nan", "room_not_last", "after_last_room", "zero_area"])
def test_relation_acc_torch_hand_made_cases(case):
    """NaN boxes (compute_rel returns None), a room row that is not last, rows behind the last room row, zero-area boxes: per
    triple against the reference's scene_graph_acc"""
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    alt = dict(vocab, pred_idx_to_name=meta["alt_pred_idx_to_name"])
    objs, boxes, tr = _t(g["case:%s:objs" % case]), _t(g["case:%s:boxes" % case]), _t(g["case:%s:triples" % case])
    for vname, voc in (("vocab", vocab), ("alt", alt)):
        k = "case:%s:%s:" % (vname, case)
        good, conf = E.relation_acc_torch(boxes[None], objs, tr, E.room_class(voc), E.relation_table(voc))
        assert int(good[0]) == int(g[k + "good"]), vname
        per = [int(E.relation_acc_torch(boxes[None], objs, tr[t:t + 1], E.room_class(voc), E.relation_table(voc))[0][0])
               for t in range(tr.shape[0])]
        assert per == g[k + "hit"].tolist(), vname


def test_confusion_table_counts_every_named_triple():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    k = "b2:"
    objs, tr, lay = _t(g[k + "objs"]), _t(g[k + "triples"]), _t(g[k + "layouts"])
    good, conf = E.relation_acc_torch(lay, objs, tr, E.room_class(vocab), E.relation_table(vocab))
    per_pred = torch.bincount(tr[:, 1], minlength=16)
    for s in range(3):
        assert conf[s].sum(1).tolist() == per_pred.tolist()
    # the in-room triples always match
    assert conf[:, 0, 0].tolist() == [int((tr[:, 1] == 0).sum())] * 3


def test_baselines_torch_replay_the_reference_draws():
    """random_scene and the perturbed layout from the recorded np.random draws: bit-identical"""
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        out = E.baselines_torch(_t(g[k + "boxes"]), _t(g[k + "objs"]), E.room_class(vocab), _t(g[k + "uniforms"]), _t(g[k + "normals"]))
        assert np.array_equal(out.numpy(), g[k + "layouts"][1:]), b


def test_l1_and_spread_torch_match_the_reference_figures():
    E = pkg("host.evaluate")
    g, meta, vocab = _fixture()
    l1s, stds = [], []
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        l1 = E.layout_l1_torch(_t(g[k + "layouts"]), _t(g[k + "boxes"])).numpy()
        # the L1 is taken before scene_graph_acc restores the layout in place: layouts[0] is the decode itself
        assert np.array_equal(g[k + "layouts"][0], g[k + "pred_boxes"])
        np.testing.assert_allclose(l1, g[k + "l1"], rtol=1e-6)
        sp = E.layout_spread_torch(_t(g[k + "std_boxes"]), _t(g[k + "std_angles"])).numpy()
        np.testing.assert_allclose(sp, g[k + "std"], rtol=1e-6)
        l1s.append(l1), stds.append(sp)
    pr = g["printed"]
    np.testing.assert_allclose(np.mean(l1s, 0), pr[0:3], rtol=1e-6)
    np.testing.assert_allclose(np.mean(stds, 0), pr[6:9], rtol=1e-6)
    tot = sum(int(g["b%d:triples" % b].shape[0]) for b in range(meta["n_batches"]))
    acc = sum(g["b%d:good" % b] for b in range(meta["n_batches"])) / tot
    np.testing.assert_allclose(acc, pr[3:6], rtol=1e-12)


def test_spread_torch_single_sample_is_zero():
    E = pkg("host.evaluate")
    b = torch.rand(1, 7, 6)
    assert E.layout_spread_torch(b, torch.zeros(1, 7, dtype=torch.int64)).tolist() == [0.0, 0.0, 0.0]


def test_mean_cov_pickle_round_trip(tmp_path):
    """the reference's stats file: a pickled [mean_est, cov_est] (testing/test_VAE.py:54-61)"""
    import pickle
    E = pkg("host.evaluate")
    g, _, _ = _fixture()
    p = os.path.join(str(tmp_path), "mean_cov.pkl")
    with open(p, "wb") as f:
        pickle.dump([g["mean"], g["cov"]], f)
    m, c = E.load_mean_cov(p)
    assert m.dtype == torch.float64 and np.array_equal(m.numpy(), g["mean"]) and np.array_equal(c.numpy(), g["cov"])
    q = os.path.join(str(tmp_path), "again.pkl")
    E.save_mean_cov(q, m, c)
    with open(q, "rb") as f:
        m2, c2 = pickle.load(f)
    assert isinstance(m2, np.ndarray) and np.array_equal(m2, g["mean"]) and np.array_equal(c2, g["cov"])


def test_device_entry_points_reject_box_dim_4_without_launching():
    """box_dim != 6 is a contract violation: a ValueError on the host side and SLN_E_BADARG from the library (no launch)"""
    E = pkg("host.evaluate")
    L = pkg("_lib")
    with pytest.raises(ValueError):
        E._check_layouts(torch.zeros(2, 3, 4))
    tab = (L.C.c_int * 16)(*range(16))
    lib = L.lib()
    assert lib.sln_layout_relation_acc(L.C.c_void_p(8), 1, 3, 4, L.C.c_void_p(8), L.C.c_void_p(8), 1, 0, tab, L.C.c_void_p(8), None, None) == -1
    assert lib.sln_layout_spread(L.C.c_void_p(8), L.C.c_void_p(8), 2, 3, 4, L.C.c_void_p(8), None) == -1
    assert lib.sln_layout_l1(L.C.c_void_p(8), 2, 3, 4, L.C.c_void_p(8), L.C.c_void_p(8), None) == -1
    assert lib.sln_layout_baselines(L.C.c_void_p(8), L.C.c_void_p(8), 3, 4, 0, L.C.c_void_p(8), L.C.c_void_p(8), None, L.C.c_void_p(8), None) == -1
