"""The refinement report on the device: sln_layout_cuboid_iou, sln_layout_overlap, sln_refine_report, RefineBatch(report=...) and
measure_acc_l1_std(overlap=True) against tests/golden/refine_report.npz (the reference's get_boxes / get_iou_cuboid and k loop executed
from its source text, tools/gen_golden_refine_report.py) and the float64 restatements of host/evaluate.py.
Tolerance: the project's standing rule (tests/parity.py: 1e-4 of the tensor's max norm + 2e-6); counts exactly."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden, pkg
from parity import assert_close

pytestmark = pytest.mark.gpu

from oracle import refine_ref, vae_ref     # noqa: E402   (the checker: table loader + configs of the fixtures)
from oracle.refine_ref import FIXTURE_VOCAB     # noqa: E402

DEV = "cuda"
LOOP_CFGS = {"refine_loop": dict(embedding_dim=32, gconv_num_layers=2, num_objs=len(FIXTURE_VOCAB) + 1),
             "refine_loop_recurrent": dict(embedding_dim=32, gconv_num_layers=3, gconv_mode="recurrent", num_objs=len(FIXTURE_VOCAB) + 1)}
LOOP_IMAGE = 96


def _meta(g):
    return json.loads(bytes(g["meta"]).decode())


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _single(n):
    return torch.full((n,), n - 1, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# sln_layout_cuboid_iou
# ------------------------------------------------------------------------------------------------------------------------------
def test_cuboid_iou_hand_cases():
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    m = _meta(g)
    for name in m["hand"]:
        p = "hand:%s:" % name
        objs = _d(g[p + "objs"])
        kept = g[p + "kept"]
        vis = E.visible_rows(objs, m["names"])
        iou, mean = E.cuboid_iou(_d(g[p + "boxes"])[None], _d(g[p + "angles"])[None], _d(g[p + "gt_boxes"]), _d(g[p + "gt_angles"]),
                                 _single(len(objs)), vis)
        print(name, iou[0].cpu().tolist(), g[p + "iou"].tolist())
        if len(kept):
            assert_close(iou[0].cpu().numpy()[kept], g[p + "iou"], "hand case " + name)
            assert_close(mean[0, 0].cpu().numpy(), np.mean(g[p + "iou"]), "mean of " + name)
        else:
            assert bool(torch.isnan(mean).all()), name                        # a room whose every object is filtered: np.mean([])


def test_cuboid_iou_random_pairs_and_layout_batches():
    """the 2 000 random pairs (100 rooms in one collated batch, per-room means), alone and as layout 1 of S = 3 / S = 257 launches whose
    other layouts are the ground truth itself"""
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    b, a, gb, ga, rr = (_d(g["rand:" + k]) for k in ("boxes", "angles", "gt_boxes", "gt_angles", "room_of_row"))
    O = b.shape[0]
    vis = torch.ones(O, dtype=torch.bool, device=DEV)
    rooms = np.unique(g["rand:room_of_row"])
    want_mean = np.asarray([g["rand:iou"][g["rand:room_of_row"] == r].mean() for r in rooms])
    for S in (1, 3, 257):
        lay, ang = gb[None].repeat(S, 1, 1), ga[None].repeat(S, 1)
        lay[S // 2], ang[S // 2] = b, a
        iou, mean = E.cuboid_iou(lay, ang, gb, ga, rr, vis)
        err = np.abs(iou[S // 2].cpu().numpy() - g["rand:iou"])
        print("S = %d: max err %.3e at row %d" % (S, err.max(), int(err.argmax())))
        assert_close(iou[S // 2].cpu().numpy(), g["rand:iou"], "2000 random pairs, S = %d" % S)
        assert_close(mean[S // 2].cpu().numpy(), want_mean, "per-room means, S = %d" % S)
        if S > 1:
            self_iou, _ = E.cuboid_iou_torch(gb.cpu()[None], ga.cpu()[None], gb.cpu(), ga.cpu(), rr.cpu())
            assert_close(iou[0].cpu().numpy(), self_iou[0].numpy(), "the ground truth against itself")
        iou2, mean2 = E.cuboid_iou(lay, ang, gb, ga, rr, vis)
        assert torch.equal(iou, iou2) and torch.equal(mean, mean2)            # fixed summation order
        _, acc = E.cuboid_iou(lay, ang, gb, ga, rr, vis, want_rows=False, mean=mean2)
        assert torch.equal(acc, 2 * mean)                                     # += into the accumulator


def test_cuboid_iou_loop_rows():
    E = pkg("host.evaluate")
    g = load_golden("refine_report")
    m = _meta(g)
    for case, n_rooms in m["loops"].items():
        lg = load_golden(case)
        for r in range(n_rooms):
            p, q = "room%d:" % r, "loop:%s:room%d:" % (case, r)
            objs = _d(lg[p + "objs"])
            iou, mean = E.cuboid_iou(_d(lg[p + "boxes"]), _d(lg[p + "idx"]), _d(lg[p + "in_boxes"]), _d(lg[p + "in_angles"], torch.float32),
                                     _single(len(objs)), E.visible_rows(objs, m["names"]))
            assert_close(iou.cpu().numpy()[:, g[q + "kept"]], g[q + "ious"], "%s room %d rows" % (case, r))
            assert_close(mean[:, 0].cpu().numpy(), g[q + "iou"], "%s room %d means" % (case, r))


def test_cuboid_iou_edge_cases():
    E, L = pkg("host.evaluate"), pkg("_lib")
    g = load_golden("refine_report")
    p = "hand:bins:"
    b, a, gb, ga = _d(g[p + "boxes"])[None].clone(), _d(g[p + "angles"])[None].clone(), _d(g[p + "gt_boxes"]), _d(g[p + "gt_angles"])
    n = b.shape[1]
    vis = torch.ones(n, dtype=torch.bool, device=DEV)
    b[0, 1, 0] = float("nan"); a[0, 2] = float("nan"); b[0, 3, 4] = float("nan")
    iou, mean = E.cuboid_iou(b, a, gb, ga, _single(n), vis)
    torch.cuda.synchronize()                                                  # NaN in, NaN out: no hang, no trap
    got = iou[0].cpu().numpy()
    assert np.isnan(got[[1, 2, 3]]).all() and np.isfinite(got[[0, 4, 5, 6]]).all() and bool(torch.isnan(mean).all())
    lib, P, st = L.lib(), L.ptr, L.current_stream_ptr()
    rr, rid, v8 = _single(n), torch.zeros(n, dtype=torch.int32, device=DEV), vis.to(torch.uint8)
    out = torch.zeros(1, 1, dtype=torch.float64, device=DEV)
    # S = 0 is a no-op, as sln_layout_l1 treats it; null pointers and bad sizes are refused without a launch
    assert lib.sln_layout_cuboid_iou(P(b), P(a), P(gb), P(ga), P(rr), P(v8), P(rid), 1, 0, n, None, P(out), st) == 0
    assert float(out) == 0.0
    assert lib.sln_layout_cuboid_iou(None, P(a), P(gb), P(ga), P(rr), P(v8), P(rid), 1, 1, n, None, P(out), st) == -1
    assert lib.sln_layout_cuboid_iou(P(b), P(a), P(gb), P(ga), P(rr), P(v8), P(rid), 1, 1, n, None, None, st) == -1
    assert lib.sln_layout_cuboid_iou(P(b), P(a), P(gb), P(ga), P(rr), None, P(rid), 1, 1, n, None, P(out), st) == -1
    assert lib.sln_layout_cuboid_iou(P(b), P(a), P(gb), P(ga), P(rr), P(v8), P(rid), 1, -1, n, None, P(out), st) == -1
    vol, prs = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.sln_layout_overlap(P(b), P(a), P(rr), P(v8), 0, n, 0.0, P(vol), P(prs), st) == 0
    assert lib.sln_layout_overlap(P(b), P(a), P(rr), None, 1, n, 0.0, P(vol), P(prs), st) == -1
    assert lib.sln_layout_overlap(P(b), P(a), P(rr), P(v8), 1, -1, 0.0, P(vol), P(prs), st) == -1
    assert float(vol) == 0.0 and int(prs) == 0
    with pytest.raises(ValueError):
        E.cuboid_iou(b, a, gb, ga, torch.zeros(n, dtype=torch.int32, device=DEV), vis)      # room rows in front of their rows


# ------------------------------------------------------------------------------------------------------------------------------
# sln_layout_overlap
# ------------------------------------------------------------------------------------------------------------------------------
def _collated(g, meta, batches):
    """rows of the eval_metrics fixture's collated batches, joined"""
    objs = np.concatenate([g["b%d:objs" % b] for b in batches])
    boxes = np.concatenate([g["b%d:boxes" % b] for b in batches])
    return torch.from_numpy(objs), torch.from_numpy(boxes)


@pytest.mark.parametrize("S", [1, 3, 257])
def test_layout_overlap_matches_the_fp64_restatement(S):
    E = pkg("host.evaluate")
    g = load_golden("eval_metrics")
    meta = _meta(g)
    names = meta["object_idx_to_name"]
    room = names.index("__room__")
    for batches in ([1], list(range(meta["n_batches"]))):                    # one collated batch, and the largest: all of them joined
        objs, gt = _collated(g, meta, batches)
        O = objs.shape[0]
        gen = torch.Generator().manual_seed(100 + S + O)
        rr, vis = E.room_rows(objs, room), E.visible_rows(objs, names)
        boxes = gt[None] + 0.08 * torch.randn(S, O, 6, generator=gen)         # furniture pushed into each other
        boxes[:, rr.long() == torch.arange(O)] = gt[rr.long() == torch.arange(O)]
        ang = torch.rand(S, O, generator=gen) * 25.0 - 1.0
        vol64, _, pair_iou = E.layout_overlap_torch(boxes, ang, rr, vis)
        # a threshold no pair's IoU lies within 1e-3 of (fp64 restatement): the middle of the widest gap between neighbouring IoUs
        flat = torch.sort(pair_iou.flatten()).values
        flat = flat[flat > 0.02]
        gaps = flat[1:] - flat[:-1]
        i = int(torch.argmax(gaps))
        thresh = float((flat[i] + flat[i + 1]) / 2)
        assert float((pair_iou - thresh).abs().min()) > 1e-3, "no clear threshold in this draw"
        want_pairs = (pair_iou > thresh).sum(1)
        vol, pairs = E.layout_overlap(boxes.to(DEV), ang.to(DEV), rr.to(DEV), vis.to(DEV), thresh=thresh)
        print("S %d O %d: pairs/layout %d, thresh %.4f, counted %s.., vol %s.." % (S, O, pair_iou.shape[1], thresh, want_pairs[:3].tolist(),
                                                                                 vol64[:3].tolist()))
        assert torch.equal(pairs.cpu(), want_pairs)
        assert_close(vol.cpu().numpy(), vol64.numpy(), "intersection volume, S = %d, O = %d" % (S, O))
        vol2, pairs2 = E.layout_overlap(boxes.to(DEV), ang.to(DEV), rr.to(DEV), vis.to(DEV), thresh=thresh)
        assert torch.equal(vol, vol2) and torch.equal(pairs, pairs2)
        assert int(want_pairs.sum()) > 0 and float(vol64.sum()) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# RefineBatch(report=...)
# ------------------------------------------------------------------------------------------------------------------------------
def _names(objs):
    return [(["__room__"] + FIXTURE_VOCAB)[int(o)] for o in objs]


def _bank(g):
    R = pkg("host.refine")
    t = refine_ref.load_tables(g)
    meshes = {k: (m["v"], m["f"], m["bbox_min"], m["bbox_max"]) for k, m in t["models"].items()}
    return R.MeshBank.from_arrays(meshes, DEV, vocab=t["vocab"], shell=t["shell"])


def _loop_model(g, case):
    M = pkg("host.Sg2ScVAE_model")
    cfg = vae_ref.VaeConfig(**LOOP_CFGS[case])
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]).clone() for k in g.files if k.startswith("state:")})
    return model.to(DEV).eval()


def _loop_rooms(g, rooms):
    out = []
    for r in rooms:
        p = "room%d:" % r
        out.append(dict(objs=_d(g[p + "objs"]), triples=_d(g[p + "triples"]), boxes=_d(g[p + "in_boxes"]), angles=_d(g[p + "in_angles"]),
                        attributes=_d(g[p + "attributes"]), class_names=_names(g[p + "objs"])))
    return out


class _Counting:
    """the loaded library behind a proxy that counts the calls of every entry point"""

    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self.real, name)


def _run(case, rooms, report, capture=False, count=None):
    """-> dict of what a run leaves behind (cpu tensors); ``count``: receives {entry point: calls} of the run() itself"""
    R = pkg("host.refine")
    Lm = pkg("_lib")
    g = load_golden(case)
    model = _loop_model(g, case)
    it = g["room0:noise"].shape[0]
    rb = R.RefineBatch(model, _loop_rooms(g, rooms), bank=_bank(g), image_size=LOOP_IMAGE, iters=it, report=report)
    try:
        for i, r in enumerate(rooms):                                        # the reference's z draw, as the loop test injects it
            a, n = rb.row0[i], rb.rows[i]
            rb.z[a:a + n] = _d(g["room%d:z0" % r])
        if count is not None:
            real = Lm.lib()
            Lm._lib = proxy = _Counting(real)
            try:
                rb.run(capture=capture)
            finally:
                Lm._lib = real
            count.append(proxy.calls)
        else:
            rb.run(capture=capture)
        torch.cuda.synchronize()
        out = dict(losses=rb.losses.cpu().clone(), boxes=rb.boxes.cpu().clone(), idx=rb.idx.cpu().clone(), z=rb.z.cpu().clone(),
                   params=rb.params.cpu().clone(), launches=rb.launches(), report=rb.report.cpu().clone() if report is not None else None)
    finally:
        rb.close()
    return out


@pytest.mark.parametrize("case,rooms", [("refine_loop", [0, 1]), ("refine_loop_recurrent", [0])])
def test_refine_batch_report(case, rooms):
    L = pkg("_lib").lib()
    g = load_golden("refine_report")
    L.sln_set_deterministic(1)
    try:
        n_none, n_all = [], []
        none = _run(case, rooms, None, count=n_none)
        none2 = _run(case, rooms, None)
        full = _run(case, rooms, "all", count=n_all)
        ends = _run(case, rooms, "ends")
        graph = _run(case, rooms, "all", capture=True)
    finally:
        L.sln_set_deterministic(0)
    it = full["report"].shape[0]
    # the report against the reference's own records, every iteration
    for i, r in enumerate(rooms):
        q = "loop:%s:room%d:" % (case, r)
        want = np.stack([g[q + "iou"], g[q + "depth_mse"], g[q + "cross_entropy"]], 1)
        got = full["report"][:, i].numpy()
        print(case, "room", r, "\n got", got.tolist(), "\nwant", want.tolist())
        for c, name in enumerate(("iou", "depth_l1", "ce_last")):
            assert_close(got[:, c], want[:, c], "%s room %d %s" % (case, r, name))
    # the report changes nothing else: bit-identical to report=None (which is bit-identical to itself)
    for k in ("losses", "boxes", "idx", "z", "params"):
        assert torch.equal(none[k], none2[k]), "deterministic mode repeats " + k
        assert torch.equal(none[k], full[k]) and torch.equal(none[k], ends[k]), k
    assert none["launches"] == full["launches"] == ends["launches"]
    # 'ends': the middle rows stay NaN, the ends equal 'all'
    assert torch.equal(ends["report"][0], full["report"][0]) and torch.equal(ends["report"][it - 1], full["report"][it - 1])
    assert bool(torch.isnan(ends["report"][1:it - 1]).all()) and not bool(torch.isnan(full["report"]).any())
    # one replayed graph: the eager report, bit for bit
    assert torch.equal(graph["report"], full["report"])
    # library calls of a run: the report adds one IoU and one report call per reported iteration and nothing else
    print("library calls of a run: report=None %s" % n_none[0])
    extra = {"sln_layout_cuboid_iou": it, "sln_refine_report": it}
    assert "sln_layout_cuboid_iou" not in n_none[0] and "sln_refine_report" not in n_none[0]
    assert n_all[0] == dict(n_none[0], **extra)


def test_refine_batch_report_arguments():
    R = pkg("host.refine")
    g = load_golden("refine_loop")
    model = _loop_model(g, "refine_loop")
    rooms, bank = _loop_rooms(g, [0]), _bank(g)
    with pytest.raises(ValueError):
        R.RefineBatch(model, rooms, bank=bank, image_size=LOOP_IMAGE, iters=4, report="some")
    with pytest.raises(ValueError):
        R.RefineBatch(model, rooms, bank=bank, image_size=LOOP_IMAGE, iters=4, report=[7])
    rb = R.RefineBatch(model, rooms, bank=bank, image_size=LOOP_IMAGE, iters=4, report=[2])
    try:
        with pytest.raises(ValueError):
            rb.run(capture=True)                                              # one graph for every iteration: 'all' or None
        rb.run()
        rep = rb.report.cpu()
        assert bool(torch.isnan(rep[[0, 1, 3]]).all()) and not bool(torch.isnan(rep[2]).any())
    finally:
        rb.close()
    two = R.finetune_vae_fast_batch(model, rooms, iters=2, bank=bank, image_size=LOOP_IMAGE)
    three = R.finetune_vae_fast_batch(model, rooms, iters=2, bank=bank, image_size=LOOP_IMAGE, report="ends")
    assert len(two) == 2 and len(three) == 3 and three[2].shape == (2, 1, 3) and not bool(torch.isnan(three[2]).any())


# ------------------------------------------------------------------------------------------------------------------------------
# measure_acc_l1_std(overlap=True)
# ------------------------------------------------------------------------------------------------------------------------------
def test_measure_overlap_leaves_the_nine_figures_alone():
    E = pkg("host.evaluate")
    M = pkg("host.Sg2ScVAE_model")
    g = load_golden("eval_metrics")
    meta = _meta(g)
    vocab = dict(object_idx_to_name=meta["object_idx_to_name"], pred_idx_to_name=meta["pred_idx_to_name"])
    cfg = vae_ref.VaeConfig(**meta["cfg"])
    sd = vae_ref.init_state(cfg, seed=meta["weight_seed"])
    model = M.Sg2ScVAEModel(**cfg.model_kwargs())
    model.load_state_dict({k: v.clone() for k, v in sd.items()})
    model = model.to(DEV).eval()
    batches, draws = [], []
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        batches.append((None, _d(g[k + "objs"]), _d(g[k + "boxes"]), _d(g[k + "triples"]), _d(g[k + "angles"]), _d(g[k + "attributes"]),
                        _d(g[k + "obj_to_img"]), None))
        draws.append(dict(z=_d(g[k + "z"]), uniforms=_d(g[k + "uniforms"], torch.float32), normals=_d(g[k + "normals"], torch.float32),
                          z_std=_d(g[k + "z_std"])))
    mean, cov = torch.from_numpy(g["mean"]), torch.from_numpy(g["cov"])
    off = E.measure_acc_l1_std(model, batches, mean, cov, vocab, n_std_samples=meta["nsample"], draws=draws)
    on = E.measure_acc_l1_std(model, batches, mean, cov, vocab, n_std_samples=meta["nsample"], draws=draws, overlap=True)
    assert len(off) == 9 and set(on) == set(off) | {"overlap_pred", "overlap_rand", "overlap_pert"}
    for k in off:
        assert on[k] == off[k], k                                             # to the last bit
    # the two baselines' layouts are in the fixture: their figure against the fp64 restatement
    names = meta["object_idx_to_name"]
    want = np.zeros(3)
    for b in range(meta["n_batches"]):
        k = "b%d:" % b
        objs = torch.from_numpy(g[k + "objs"])
        rr, vis = E.room_rows(objs, names.index("__room__")), E.visible_rows(objs, names)
        ang = torch.from_numpy(g[k + "angles"]).double()[None].repeat(3, 1)
        want += E.layout_overlap_torch(torch.from_numpy(g[k + "layouts"]), ang, rr, vis)[0].numpy() / meta["n_batches"]
    print("overlap", on["overlap_pred"], on["overlap_rand"], on["overlap_pert"], "fp64 of the fixture's layouts", want.tolist())
    assert_close(np.asarray([on["overlap_rand"], on["overlap_pert"]]), want[1:], "overlap of the replayed baselines")
    assert on["overlap_pred"] >= 0.0 and np.isfinite(on["overlap_pred"])
