"""Operands of the refinement-loss family (test_refine_loss_cases_host.py, test_refine_loss_family_gpu.py): sign-safe images at the
smallest geometries at which every route and edge of csrc/refine_loss.hip exists, and their fp64 / fp32 reference evaluations.

The L1 part of the loss has the gradient sign(pooled difference) * const: an image pair whose pooled differences come close to 0 makes
the gradient of any fp32 evaluation differ from the fp64 one by a whole step, and a test on it has to leave elements out.  Here no
pooled difference comes closer to 0 than 0.05, so EVERY gradient element is compared:

  depth planes     iterate = target + sign[b, c] * delta, delta in [0.05, 0.25] per pixel, target in [0.3, 0.7]; the sign is constant per
                   (image, plane) and + on the last plane.  Both resampling stages are convex combinations: a pooled difference keeps the
                   plane's sign and a magnitude >= 0.05.
  null region      a corner block of the iterate: its depth values lie in [0, 0.01] (sum <= 0.29 < 0.5), target = iterate - sign * delta
                   there; the last plane's filled value 1 keeps the + difference.  Elsewhere the depth sum is >= n_dep * 0.05 >= 0.55.
  semantic planes  target: a blocky label map, plane c = 0.6 + 0.01 * c inside the blocks of class c, with an empty corner (label -100);
                   iterate: randn.  The seeds are those at which the pooled map keeps the margins of the host test (a pooled pixel
                   at the rim of the empty corner can land anywhere between 0 and 0.6).
  plane 0          arbitrary in both.

Everything is drawn in fp64 from the case's seed and rounded to fp32 once: the fp64 reference, the fp32 yardstick and the device see
the same numbers.  What has to hold for the comparison of every element (margins of the pooled differences, of the depth sums, of the
labels) is asserted per case by test_refine_loss_cases_host.py, on the CPU, from the reference alone."""
import functools

import numpy as np
import torch

from conftest import pkg
from oracle import refine_ref

import refine_mask_cases as MC

# S, sizes -> (pooling kernel, backward kernel, longest CSR row): the route table of LAB_NOTES.md, asserted by the host test from the
# host-side tables with the launchers' own rules
GEOMETRIES = {
    "s40_3scales": dict(S=40, sizes=(8, 12, 16), pool="lds", backward="separable", max_col=4, report=True, rooms_ok=True),
    "s264_2blocks": dict(S=264, sizes=(8, 16), pool="lds", backward="separable", max_col=4, report=True, rooms_ok=True),
    "s24_upsample": dict(S=24, sizes=(100, 16), pool="plain", backward="separable", max_col=2, report=True, rooms_ok=True),
    "s40_p104": dict(S=40, sizes=(8, 104), pool="plain", backward="generic", max_col=26, report=False, rooms_ok=True),
    "s40_generic": dict(S=40, sizes=(12, 20, 32), pool="lds", backward="generic", max_col=6, report=True, rooms_ok=True),
    "s36_tail": dict(S=36, sizes=(30,), pool="lds", backward="separable", max_col=2, report=False, rooms_ok=False),
    "s96_workload": dict(S=96, sizes=(32, 48, 64, 96), pool="lds", backward="separable", max_col=5, report=True, rooms_ok=True),
}
POOL_LDS_MAX, SEP_MAX_ENTRIES, SEP_MAX_P = 96, 5, 96          # launch_pool's and sln_refine_loss_backward's thresholds


def _case(name, geometry, B=1, per_room=False, mask=None, C=70, extra_channels=0, seed=0):
    return dict(name=name, geometry=geometry, B=B, per_room=per_room, mask=mask, C=C, extra_channels=extra_channels, seed=seed, **GEOMETRIES[geometry])


# mask: None, or one pattern name of refine_mask_cases per room ("zeros" alone: the all-invalid case)
CASES = [
    _case("s40-b1", "s40_3scales", seed=1),
    _case("s40-b3-rooms", "s40_3scales", B=3, per_room=True, seed=2),
    _case("s40-b3-batch-mask", "s40_3scales", B=3, mask=("rectangle", "random", "ones"), seed=3),
    _case("s40-b3-rooms-mask", "s40_3scales", B=3, per_room=True, mask=("row", "corner00", "rectangle"), seed=4),
    _case("s40-b1-all-invalid", "s40_3scales", mask=("zeros",), seed=5),
    _case("s40-ndep11-b3", "s40_3scales", B=3, C=52, extra_channels=2, seed=106),
    _case("s40-ndep11-b1-rooms-mask", "s40_3scales", per_room=True, mask=("random",), C=52, extra_channels=2, seed=7),
    _case("s264-b1", "s264_2blocks", seed=208),
    _case("s264-b1-rooms-mask", "s264_2blocks", per_room=True, mask=("rectangle",), seed=9),
    _case("s24-b3-batch", "s24_upsample", B=3, seed=10),
    _case("s24-b1-rooms", "s24_upsample", per_room=True, seed=11),
    _case("s24-b3-rooms-mask", "s24_upsample", B=3, per_room=True, mask=("interior", "rectangle", "cornerSS"), seed=12),
    _case("p104-b1", "s40_p104", seed=1313),
    _case("p104-b3-rooms", "s40_p104", B=3, per_room=True, seed=2414),
    _case("p104-b1-mask", "s40_p104", mask=("rectangle",), seed=915),
    _case("generic-b1", "s40_generic", seed=16),
    _case("generic-b3-batch", "s40_generic", B=3, seed=17),
    _case("generic-b3-rooms-mask", "s40_generic", B=3, per_room=True, mask=("random", "row", "ones"), seed=618),
    _case("tail-b1", "s36_tail", seed=19),
    _case("tail-b3-batch", "s36_tail", B=3, seed=20),
    _case("tail-b3-batch-mask", "s36_tail", B=3, mask=("rectangle", "ones", "random"), seed=21),
    _case("workload-b1", "s96_workload", seed=622),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = [c["name"] for c in CASES]


def is_all_invalid(case):
    return case["mask"] == ("zeros",)


@functools.lru_cache(maxsize=None)
def host_tables(S, sizes):
    """(stage1_stride, pooled_size, max_col_entries, pooling kernel, backward kernel) of a geometry: ``RefineLoss._build_tables`` on the CPU
    and the two launchers' rules (launch_pool, sln_refine_loss_backward)"""
    R = pkg("host.refine")
    _, max_col = R.RefineLoss._build_tables(S, sizes, "cpu")
    stride, P = max(sizes), sizes[-1]
    pool = "lds" if stride <= POOL_LDS_MAX and P <= POOL_LDS_MAX else "plain"
    backward = "separable" if 0 < max_col <= SEP_MAX_ENTRIES and P <= SEP_MAX_P else "generic"
    return stride, P, max_col, pool, backward


def route(case):
    """the line a GPU case prints: which kernels its launches take"""
    _, _, max_col, pool, backward = host_tables(case["S"], case["sizes"])
    return "pool %s, backward %s (max_col %d), loss rows %d x %d scales%s, n_dep %d" % (
        pool, backward, max_col, case["sizes"][-1] ** 2, len(case["sizes"]), ", per_room" if case["per_room"] else "", case["C"] - 41)


def null_block(S):
    """the corner block of the iterate without depth: rows [0, S // 4), columns [S - S // 3, S)"""
    return slice(0, S // 4), slice(S - S // 3, S)


@functools.lru_cache(maxsize=None)
def operands(name):
    """-> dict(target, image [B, C, S, S] float32 (the target with NaN under the mask), valid [B, S, S] uint8 or None, sign [B, n_dep],
    null [B, S, S] bool).  Shared between the tests: do not write into the tensors."""
    c = BY_NAME[name]
    B, C, S = c["B"], c["C"], c["S"]
    nd = C - 41
    g = torch.Generator().manual_seed(1000 + c["seed"])
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    target, image = torch.zeros(B, C, S, S, dtype=torch.float64), torch.zeros(B, C, S, S, dtype=torch.float64)
    # depth planes
    sign = (torch.randint(0, 2, (B, nd), generator=g) * 2 - 1).double()
    sign[:, -1] = 1.0
    delta = 0.05 + 0.2 * rand(B, nd, S, S)
    step = sign[:, :, None, None] * delta
    target[:, 41:] = 0.3 + 0.4 * rand(B, nd, S, S)
    image[:, 41:] = target[:, 41:] + step
    ry, rx = null_block(S)
    image[:, 41:, ry, rx] = 0.01 * rand(B, nd, S, S)[:, :, ry, rx]
    target[:, 41:, ry, rx] = image[:, 41:, ry, rx] - step[:, :, ry, rx]
    null = torch.zeros(B, S, S, dtype=torch.bool)
    null[:, ry, rx] = True
    # semantic planes: blocks of 5 x 7 pixels, one class each; the lower left corner block stays empty.  One map per case: room 1 shows
    # its transpose and room 2 its point reflection - both resampling stages commute with either, so that the label margins the host test
    # asserts are those of room 0 while every room has labels of its own
    by, bx = 5, 7
    ny, nx = (S + by - 1) // by, (S + bx - 1) // bx
    cls = torch.randint(0, 40, (ny, nx), generator=g)
    cls = cls.repeat_interleave(by, 0).repeat_interleave(bx, 1)[:S, :S]
    amp = 0.6 + 0.01 * torch.arange(40, dtype=torch.float64)
    sem0 = torch.zeros(40, S, S, dtype=torch.float64)
    sem0.scatter_(0, cls[None], amp[cls][None])
    sem0[:, S - S // 3:, :S // 4] = 0.0
    sem = torch.stack([(sem0, sem0.transpose(1, 2), sem0.flip(1, 2))[b % 3] for b in range(B)])
    target[:, 1:41] = sem
    image[:, 1:41] = torch.randn(B, 40, S, S, generator=g, dtype=torch.float64)
    target[:, 0] = rand(B, S, S)
    image[:, 0] = torch.randn(B, S, S, generator=g, dtype=torch.float64)
    target, image = target.float(), image.float()
    valid = None
    if c["mask"] is not None:
        assert len(c["mask"]) == B
        valid = torch.from_numpy(np.stack([MC.pattern(p, S) for p in c["mask"]]))
        target = torch.where((valid != 0)[:, None], target, torch.full_like(target, float("nan")))
    return dict(target=target, image=image, valid=valid, sign=sign, null=null)


def clean_target(ops):
    """the target with 0 in place of what lies under the mask (no valid pooled pixel reads it)"""
    if ops["valid"] is None:
        return ops["target"]
    return torch.where((ops["valid"] != 0)[:, None], ops["target"], torch.zeros_like(ops["target"]))


def pooled(image, sizes, null_fill, dtype):
    """fp64 / fp32 ``psp_pool`` of planes 1.. of an image -> [B, n_scales, C - 1, P, P], sln_refine_pool's layout"""
    x = image.to(dtype).clone()
    if null_fill:
        x[:, -1][torch.sum(x[:, 41:], dim=1) < 0.5] = 1.0
    return torch.stack(refine_ref.psp_pool(x[:, 1:], sizes, as_list=True), 1)


def labels_of(target, sizes, dtype):
    """[B, n_scales, P, P] int64 labels (-100: none) of ``refine_ref.target_labels`` evaluated in ``dtype``"""
    return torch.cat(refine_ref.target_labels(target.to(dtype), sizes), 1)


def masked_labels(name, dtype=torch.float64):
    """what the loss trains against: the target's labels, -100 at invalid pooled pixels; and the pooled validity (None without a mask)"""
    c, ops = BY_NAME[name], operands(name)
    lab = labels_of(clean_target(ops), c["sizes"], dtype)
    if ops["valid"] is None:
        return lab, None
    R = pkg("host.refine")
    vp = R.valid_pooled_torch(ops["valid"], c["sizes"])
    return torch.where(vp, lab, torch.full_like(lab, -100)), vp


def _loss(case, image, target, labels, valid):
    R = pkg("host.refine")
    zero = torch.zeros((), dtype=image.dtype)
    container = [labels[:, k:k + 1] for k in range(labels.shape[1])]
    if valid is not None:
        return R.refinement_loss_masked(image, target, container, zero, valid, sizes=case["sizes"])
    return refine_ref.refinement_loss(image, target, container, zero, sizes=case["sizes"])


def evaluate(name, dtype):
    """(losses [3] or [B, 3] under per_room, d total / d image [B, C, S, S]) of the reference in ``dtype``: ``refine_ref.refinement_loss``,
    ``host.refine.refinement_loss_masked`` under a mask; per_room: one evaluation per room, each back-propagated with weight 1.  The labels
    are the fp64 ones in both types (the host test asserts that the fp32 ones are the same)."""
    c, ops = BY_NAME[name], operands(name)
    labels, _ = masked_labels(name)
    x = ops["image"].to(dtype).requires_grad_(True)
    tgt = ops["target"].to(dtype)
    valid = ops["valid"]
    rooms = [slice(b, b + 1) for b in range(c["B"])] if c["per_room"] else [slice(0, c["B"])]
    out = []
    for r in rooms:
        triple = _loss(c, x[r], tgt[r], labels[r], None if valid is None else valid[r])
        triple[0].backward()
        out.append(torch.stack([t.detach() for t in triple]))
    return (torch.stack(out) if c["per_room"] else out[0]), x.grad.detach()


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(loss64, grad64, loss32, grad32), computed once per case"""
    l64, g64 = evaluate(name, torch.float64)
    l32, g32 = evaluate(name, torch.float32)
    return dict(loss64=l64, grad64=g64, loss32=l32, grad32=g32)


def report_reference(name, dtype=torch.float64):
    """[B, 2] (depth_l1, ce_last) of sln_refine_report (include/sln_hip.h): the full-resolution L1 of the null-filled iterate against the
    target over the valid pixels, and the last scale's cross-entropy over the labels that are left; 0 for a room without a term"""
    import torch.nn.functional as F
    c, ops = BY_NAME[name], operands(name)
    labels, _ = masked_labels(name)
    x, tgt = ops["image"].to(dtype).clone(), clean_target(ops).to(dtype)
    x[:, -1][torch.sum(x[:, 41:], dim=1) < 0.5] = 1.0
    valid = ops["valid"] if ops["valid"] is not None else torch.ones(c["B"], c["S"], c["S"], dtype=torch.uint8)
    last = refine_ref.psp_pool(x[:, 1:41], c["sizes"], as_list=True)[-1]
    out = torch.zeros(c["B"], 2, dtype=dtype)
    for b in range(c["B"]):
        v = valid[b] != 0
        n = int(v.sum())
        if n:
            out[b, 0] = (x[b, 41:] - tgt[b, 41:]).abs()[:, v].sum() / ((c["C"] - 41) * n)
        if bool((labels[b, -1] >= 0).any()):
            out[b, 1] = F.cross_entropy(last[b:b + 1], labels[b:b + 1, -1])
    return out
