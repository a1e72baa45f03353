"""Posterior statistics and batched layout sampling on the device - the tensor work of the reference's
``testing/test_VAE.py`` (:34-117) and ``testing/test_heatmap.py`` (:52-64) without the per-room Python loops.

  * ``posterior_stats``  - mean / covariance of the encoder means over a set of batches (test_VAE.py:34-54; the
    reference accumulates n outer products in a numpy loop);
  * ``sample_layouts``   - ``Nsample`` decodes of the same scene graphs in ONE engine call: the graph batch is
    replicated ``n_samples`` times with shifted row ids (the decoder only sees disjoint graphs), z is drawn from
    N(mean, cov) per object as ``np.random.multivariate_normal`` does (test_VAE.py:83-84), BatchNorm runs on its
    running statistics (``model.eval()``).
"""
import contextlib
import ctypes as C

import torch

from .. import _lib


@contextlib.contextmanager
def _precision(model, precision):
    """``precision`` (None: the model's own ``gemm_precision``) for the span of one call; the previous mode comes back even when
    the call raises."""
    if precision is None:
        yield
        return
    was = model.gemm_precision
    model.gemm_precision = precision
    try:
        yield
    finally:
        model.gemm_precision = was


def posterior_stats(model, batches, precision=None):
    """batches: iterable of (objs, triples, boxes, angles, attributes).  -> (mean [E], cov [E,E]) float64 on the CPU.
    ``precision``: ``model.gemm_precision`` for this call (None: as the model is set)."""
    mus = []
    was_training = model.training
    model.eval()
    with _precision(model, precision), torch.no_grad():
        for objs, triples, boxes, angles, attributes in batches:
            mu, _ = model.encoder(objs, triples, boxes, angles, attributes)
            mus.append(mu.double())
    model.train(was_training)
    m = torch.cat(mus, 0)
    mean = m.mean(0)
    c = m - mean
    cov = c.t().matmul(c) / (m.shape[0] - 1.0)
    return mean.cpu(), cov.cpu()


def replicate_graphs(objs, triples, attributes, n):
    """n shifted copies of a collated batch (suncg_collate_fn layout): rows of copy k are offset by k*O."""
    O = objs.shape[0]
    off = (torch.arange(n, device=objs.device) * O)
    tr = triples[None].repeat(n, 1, 1)
    tr[:, :, 0] += off[:, None]
    tr[:, :, 2] += off[:, None]
    return objs.repeat(n), tr.reshape(-1, 3), attributes.repeat(n)


_REPLICAS = {}          # (objs ptr / version, triples ptr / version, attributes ptr / version, n) -> replicated graph tensors
_FACTORS = {}           # (cov ptr / version, mean ptr / version, device) -> (Cholesky factor, mean) on the device


def _replicated(objs, triples, attributes, n):
    """``replicate_graphs`` once per (graph, n): the same tensors come back on the next call, so the model keeps its bound
    batch (no CSR rebuild: a 20 000-sample heat map of one scene binds its 120 000-row graph once)."""
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in (objs, triples, attributes)) + (int(n),)
    hit = _REPLICAS.get(key)
    if hit is None:
        if len(_REPLICAS) > 8:
            _REPLICAS.clear()
        hit = _REPLICAS[key] = replicate_graphs(objs, triples, attributes, n) + ((objs, triples, attributes),)     # keep the sources alive: the key holds their addresses
    return hit[:3]


def _factor(mean, cov, E, dev):
    key = (cov.data_ptr(), cov._version, mean.data_ptr(), mean._version, str(dev))
    hit = _FACTORS.get(key)
    if hit is None:
        if len(_FACTORS) > 8:
            _FACTORS.clear()
        L = torch.linalg.cholesky(cov.double().cpu() + 1e-9 * torch.eye(E, dtype=torch.float64)).float().to(dev).contiguous()
        hit = _FACTORS[key] = (L, mean.float().to(dev).contiguous(), (mean, cov))
    return hit[:2]


def sample_layouts(model, objs, triples, attributes, n_samples=4, mean=None, cov=None, generator=None, z=None, precision=None):
    """-> boxes_pred [n_samples, O, box_dim], angle_bins [n_samples, O] (argmax of the log-probabilities), z [n_samples, O, E].

    The N(0,1) draw behind z comes from the DEVICE (the engine's Philox stream, ``model.manual_seed``) unless a CPU
    ``generator`` is passed (reproducible against a host-side reference) or ``z`` [n_samples * O, E] is injected;
    z = mean + eps L^T with the Cholesky factor of ``cov`` is one GEMM of the engine's own family (sln_linear_forward), fp32 in
    every mode.  ``precision``: ``model.gemm_precision`` for the decode of this call (None: as the model is set)."""
    dev = objs.device
    E, O = model.embedding_dim, objs.shape[0]
    ro, rt, ra = _replicated(objs, triples, attributes, n_samples)
    was_training = model.training
    model.eval()
    if z is None:
        if generator is not None:
            eps = torch.randn(n_samples * O, E, generator=generator, device="cpu").to(dev)
        else:
            model._set_batch(ro, rt, None, None, ra)                      # the engine (and its Philox stream) exists from here on
            eps = model.device_randn(n_samples * O, E)
        if mean is None:
            z = eps
        else:
            L, mu = _factor(mean, cov, E, dev)
            z = torch.empty_like(eps)
            _lib.check(_lib.lib().sln_linear_forward(_lib.ptr(eps), eps.shape[0], E, _lib.ptr(L), _lib.ptr(mu), _lib.ptr(z), E, None, -1,
                                                     _lib.current_stream_ptr()), "sln_linear_forward")
    try:
        with _precision(model, precision), torch.no_grad():
            bp, ap = model.decoder(z, ro, rt, ra)
    finally:
        model.train(was_training)
    return bp.view(n_samples, O, -1), ap.view(n_samples, O, -1).argmax(2), z.view(n_samples, O, E)


def layout_counts(boxes_pred, container_size=100, clip_coor=True, out=None):
    """The accumulation of testing/test_heatmap.py:80-99 as ONE launch (sln_layout_heatmap): -> counts [O-1, cs, cs] (+= into
    ``out``).  ``layout_heatmap`` below is the same computation in torch ops (CPU tensors, the host-side test)."""
    n, O, bd = boxes_pred.shape
    counts = out if out is not None else torch.zeros(O - 1, container_size, container_size, dtype=torch.float32, device=boxes_pred.device)
    _lib.check(_lib.lib().sln_layout_heatmap(_lib.ptr(boxes_pred.contiguous()), n, O, bd, container_size, int(clip_coor), _lib.ptr(counts),
                                             _lib.current_stream_ptr()), "sln_layout_heatmap")
    return counts


def layout_heatmap(boxes_pred, container_size=100, clip_coor=True):
    """testing/test_heatmap.py:80-99 for all objects at once: ``boxes_pred`` [n_trials, O, 6] (room row last) ->
    [O-1, container_size, container_size] histograms of the object centres in the room's own frame, each normalised
    to sum 1 (``container[rd[2], rd[0]] += 1`` per trial, then ``/ max(sum, 1)``)."""
    n, O, _ = boxes_pred.shape
    room = boxes_pred[:, -1:, :]
    ext = room[..., 3:] - room[..., :3]
    b = boxes_pred[:, :-1, :] * torch.cat([ext, ext], -1)
    ct = (b[..., :3] + b[..., 3:]) * 0.5
    if clip_coor:
        keep = torch.ones(ct.shape[:2], dtype=torch.bool, device=ct.device)
        ct = ct.clamp(0.0, 1.0)
    else:
        keep = ((ct > 0.0) & (ct < 1.0)).all(-1)
        ct = ct.clamp(0.0, 1.0)
    rd = torch.floor(ct * (container_size - 1)).long()
    flat = (torch.arange(O - 1, device=ct.device)[None] * container_size + rd[..., 2]) * container_size + rd[..., 0]
    hist = torch.zeros((O - 1) * container_size * container_size, dtype=torch.float32, device=ct.device)
    hist.scatter_add_(0, flat.reshape(-1), keep.reshape(-1).float())
    hist = hist.view(O - 1, container_size, container_size)
    return hist / hist.sum((1, 2), keepdim=True).clamp(min=1.0)


RELATIONSHIPS = ['__in_room__', 'left of', 'right of', 'behind', 'in front of', 'inside', 'surrounding', 'left touching', 'right touching',
                 'front touching', 'behind touching', 'front left', 'front right', 'back left', 'back right', 'on']
VALID_CLASSES = ["__room__", "curtain", "shower_curtain", "dresser", "counter", "bookshelf", "picture", "mirror", "floor_mat", "chair", "sink",
                 "desk", "table", "lamp", "door", "clothes", "person", "toilet", "cabinet", "floor", "window", "blinds", "wall", "pillow",
                 "whiteboard", "bathtub", "television", "night_stand", "sofa", "refridgerator", "bed", "shelves"]


def scene_graph_from_words(objs_in_scene, rels_in_scene, valid_classes=None, device="cpu"):
    """testing/test_utils.py:43-90: ``["bed", "desk", "chair:1", ...]`` + ``[("bed", "behind", "desk"), ...]`` ->
    (objs [n+1], triples [r+n, 3], attributes [n+1]) with the '__room__' row and the in-room triples appended."""
    classes = VALID_CLASSES if valid_classes is None else list(valid_classes)
    objs = [classes.index(name.split(":")[0]) for name in objs_in_scene]
    triples = [[objs_in_scene.index(s), RELATIONSHIPS.index(p), objs_in_scene.index(o)] for s, p, o in rels_in_scene]
    triples += [[i, 0, len(objs_in_scene)] for i in range(len(objs_in_scene))]
    objs.append(0)
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=device)
    return t(objs), t(triples).reshape(-1, 3), torch.zeros(len(objs), dtype=torch.int64, device=device)


_WORD_GRAPHS = {}


def heatmap_from_words(model, objs_in_scene, rels_in_scene, mean, cov, num_iter=20000, chunk=None, container_size=100, generator=None,
                       precision=None):
    """testing/test_heatmap.py:52-99 without the 20 000 single-graph decodes: ``chunk`` posterior samples of the scene (default: all
    of them) are decoded per engine call (replicated disjoint graphs) and accumulated into the per-object centre histograms on the
    device: z drawn there, one histogram launch per chunk, nothing crosses the bus but the result."""
    dev = next(model.parameters()).device
    gkey = (tuple(objs_in_scene), tuple(rels_in_scene), str(dev))
    if gkey not in _WORD_GRAPHS:
        if len(_WORD_GRAPHS) > 8:
            _WORD_GRAPHS.clear()
        _WORD_GRAPHS[gkey] = scene_graph_from_words(objs_in_scene, rels_in_scene, device=dev)
    objs, triples, attrs = _WORD_GRAPHS[gkey]
    chunk = num_iter if chunk is None else chunk
    counts, done = None, 0
    while done < num_iter:
        n = min(chunk, num_iter - done)
        bp, _, _ = sample_layouts(model, objs, triples, attrs, n_samples=n, mean=mean, cov=cov, generator=generator, precision=precision)
        counts = layout_counts(bp, container_size, True, out=counts)
        done += n
    return counts / counts.sum((1, 2), keepdim=True).clamp(min=1.0)


def footprints_from_words(model, objs_in_scene, rels_in_scene, mean, cov, num_iter=20000, chunk=None, size=100, generator=None,
                          precision=None):
    """``heatmap_from_words`` with footprints instead of centres: ``num_iter`` posterior samples of the scene are decoded in chunks and
    every object's rotated footprint (the ring testing/test_plot2d.py:88-110 draws, with the decoded angle bin) is accumulated on the
    device (``plot2d.layout_footprints``) -> counts [n + 1, size, size] int32: per object row and pixel the number of samples that
    cover it.  The planes of rows that plot2d does not draw (the room row, do_not_vis classes) stay 0."""
    from . import plot2d as _P
    dev = next(model.parameters()).device
    gkey = (tuple(objs_in_scene), tuple(rels_in_scene), str(dev))
    if gkey not in _WORD_GRAPHS:
        if len(_WORD_GRAPHS) > 8:
            _WORD_GRAPHS.clear()
        _WORD_GRAPHS[gkey] = scene_graph_from_words(objs_in_scene, rels_in_scene, device=dev)
    objs, triples, attrs = _WORD_GRAPHS[gkey]
    O = objs.shape[0]
    rank, _ = _P.plot_tables(objs, VALID_CLASSES)
    rr = torch.full((O,), O - 1, dtype=torch.int32, device=dev)
    chunk = num_iter if chunk is None else chunk
    counts, done = None, 0
    while done < num_iter:
        n = min(chunk, num_iter - done)
        bp, ab, _ = sample_layouts(model, objs, triples, attrs, n_samples=n, mean=mean, cov=cov, generator=generator, precision=precision)
        counts = _P.layout_footprints(bp, ab, rr, rank, size=size, counts=counts)
        done += n
    return counts
