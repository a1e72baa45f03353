"""Input / output side of ``colorize_with_spade`` (reference testing/test_SPADE_shade.py:16-79): the 41-channel tensor the
generator consumes and the many-z colourisation of one room.

  * ``build_input``  - depth normalisation (:50-55), class-mask stacking / thresholding at 120 (:56-70) and
    ``skimage.transform.resize(total, [256,256], preserve_range=True, order=3, anti_aliasing=True)`` (:73) as device tensor
    ops.  The resize is a fixed linear operator per axis - Gaussian anti-aliasing (sigma (f-1)/2, mirror boundary, 4 sigma
    support), cubic B-spline prefilter (mirror boundary), evaluation at the pixel centres of the coarse grid - so it is built
    once as an [out, in] matrix R in float64 and applied as ``R @ X @ R^T`` to all 41 channels at once.  scikit-image is not
    part of this image: the matrix follows its documented algorithm (scipy.ndimage gaussian_filter + zoom(grid_mode=True))
    and is tested against scipy.ndimage itself.
  * ``colorize``     - ``num_z`` images of one map in ONE generator call (gamma/beta shared, SPADEGenerator4.forward with a
    single-row ``seg``) instead of ``num_z`` batch-1 calls (:74-79); ``to_uint8`` is ``save_color``'s conversion (:16-27).
  * ``InputBuilder`` - the same tensor from csrc/spade_input.hip: depth statistics, normalisation, thresholding (or the one-hot
    expansion of a class-index image) and the resize in three launches that read the depth and one byte per pixel of every mask that
    is present, apply the resize from a banded table (``band_table``) and never form the full-resolution stack.  ``build_inputs`` is its
    convenience form, ``colorize_rooms`` shades a list of rooms with it.  ``build_input`` stays as the ATen restatement the tests hold
    the kernels to.
File reading (.exr / .png through imageio, :45-58) stays with the caller.
"""
import functools

import numpy as np
import torch

from .. import _lib as L

NYU40 = ['wall', 'floor', 'cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture',
         'counter', 'blinds', 'desk', 'shelves', 'curtain', 'dresser', 'pillow', 'mirror', 'floor_mat',
         'clothes', 'ceiling', 'books', 'refridgerator', 'television', 'paper', 'towel', 'shower_curtain',
         'box', 'whiteboard', 'person', 'night_stand', 'toilet', 'sink', 'lamp', 'bathtub', 'bag',
         'otherstructure', 'otherfurniture', 'otherprop']


def class_of(basename):
    """class name encoded in a mask file name '<a>_<b>_<c>_<class>[_<class2>].png' (:60-66)"""
    parts = basename.split(".")[0].split("_")
    return parts[3] + "_" + parts[4] if len(parts) == 5 else parts[3]


def _mirror(i, n):
    if n == 1:
        return 0
    p = 2 * (n - 1)
    i = i % p
    return i if i < n else p - i


@functools.lru_cache(maxsize=8)
def resize_matrix(n_in, n_out):
    """[n_out, n_in] float64: anti-aliased cubic-spline resize of one axis (see the module docstring)."""
    f = n_in / n_out
    if n_in == n_out:
        return np.eye(n_in)
    sigma = max(0.0, (f - 1) / 2)
    G = np.eye(n_in)
    if sigma > 0:
        lw = int(4.0 * sigma + 0.5)
        w = np.exp(-0.5 * (np.arange(-lw, lw + 1) / sigma) ** 2); w /= w.sum()
        G = np.zeros((n_in, n_in))
        for i in range(n_in):
            for k, wk in zip(range(-lw, lw + 1), w):
                G[i, _mirror(i + k, n_in)] += wk
    C = np.zeros((n_in, n_in))                                  # cubic B-spline collocation, whole-sample mirror boundary
    for i in range(n_in):
        C[i, i] += 4.0 / 6.0
        C[i, _mirror(i - 1, n_in)] += 1.0 / 6.0
        C[i, _mirror(i + 1, n_in)] += 1.0 / 6.0
    P = np.linalg.inv(C)
    S = np.zeros((n_out, n_in))
    for o in range(n_out):
        x = (o + 0.5) * f - 0.5                                  # grid_mode: pixel centres of the coarse grid
        k = int(np.floor(x)); t = x - k
        wts = [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]
        for j, wj in zip(range(k - 1, k + 3), wts):
            S[o, _mirror(j, n_in)] += wj
    return S @ P @ G


def normalise_depth(depth):
    d = depth.float()
    d = d - d.min()
    dmax = d[d < 20].max()
    d = d.clamp(0, float(dmax)) / dmax
    return (d - 0.5) * 2


def build_input(depth, masks, size=256, device=None):
    """depth [H,W] (first channel of the .exr), masks {class name: [H,W] tensor 0..255} -> [1,41,size,size] float32."""
    dev = device or depth.device
    depth = depth.to(dev)
    H, W = depth.shape
    total = torch.zeros(41, H, W, dtype=torch.float32, device=dev)
    total[0] = normalise_depth(depth)
    for name, m in masks.items():
        m = m.to(dev).float()
        total[1 + NYU40.index(name)] = torch.where(m < 120, torch.zeros_like(m), torch.where(m > 120, torch.ones_like(m), m))
    Rh = torch.from_numpy(resize_matrix(H, size)).to(dev)
    Rw = torch.from_numpy(resize_matrix(W, size)).to(dev)
    out = torch.matmul(torch.matmul(Rh, total.double()), Rw.t())   # float64 like skimage's internal image
    return out.float()[None].contiguous()


def colorize(model, total, num_z, generator=None):
    """-> [num_z, 3, S, S] in (-1, 1): ``num_z`` z ~ N(0,1) for the ONE map ``total`` [1,41,S,S] (:36-38, :74-79)."""
    z = torch.randn(num_z, model.nz, device=total.device, generator=generator)
    return model(total, z)


def to_uint8(images):
    """save_color's conversion (:16-27): [N,3,S,S] in [-1,1] -> uint8 [N,S,S,3]"""
    a = (images.detach().float() + 1.0) / 2.0
    return (a.permute(0, 2, 3, 1) * 255.0).to(torch.uint8)


@functools.lru_cache(maxsize=8)
def band_table(n_in, n_out, eps=1e-12):
    """``resize_matrix(n_in, n_out)`` as a band: (first [n_out] int32, weights [n_out, width] float64) with
    ``R[o, first[o] + k] ~ weights[o, k]``.  ``width`` is the longest run, over the rows, from the first to the last entry with
    ``|R| > eps``; a row whose own run is shorter (or would end behind ``n_in``) is filled with its true neighbouring entries, so
    every entry left out is ``<= eps`` in magnitude."""
    R = resize_matrix(n_in, n_out)
    big = np.abs(R) > eps
    lo = big.argmax(1)
    hi = n_in - 1 - big[:, ::-1].argmax(1)
    width = int((hi - lo + 1).max())
    first = np.minimum(lo, n_in - width).astype(np.int32)
    weights = np.ascontiguousarray(R[np.arange(n_out)[:, None], first[:, None] + np.arange(width)[None, :]])
    return first, weights


def masks_from_labels(labels):
    """class-index image [H,W] (0: no class, 1 + c: NYU class c) -> {class name: uint8 mask [H,W] of 0 / 255} of the classes present"""
    labels = torch.as_tensor(labels)
    return {NYU40[c - 1]: (labels == c).to(torch.uint8) * 255 for c in torch.unique(labels).tolist() if c > 0}


def labels_from_masks(masks, shape=None):
    """{class name: mask [H,W] 0..255} of DISJOINT masks (> 120 is inside) -> uint8 class-index image; the inverse of
    ``masks_from_labels``"""
    masks = {k: torch.as_tensor(v) for k, v in masks.items()}
    first = next(iter(masks.values())) if masks else None
    labels = torch.zeros(tuple(shape) if first is None else first.shape, dtype=torch.uint8, device=None if first is None else first.device)
    for name, m in masks.items():
        inside = m > 120
        if bool((labels[inside] != 0).any()):
            raise ValueError("masks overlap at class %r: a class-index image holds one class per pixel" % name)
        labels[inside] = 1 + NYU40.index(name)
    return labels


class InputBuilder:
    """[B,41,size,size] float32 from ``B`` rooms of [H,W] file arrays, on the device (csrc/spade_input.hip).

        builder = InputBuilder(1024, 1024, device="cuda")
        total = builder(depth, masks=planes, channels=["bed", "wall"])      # planes [2,H,W] uint8 (a PNG's bytes) or float32
        total = builder(depth, labels=class_index_image)                    # uint8 [H,W]: 0 no class, 1 + c NYU class c

    With ``batch`` > 1 the arrays carry a leading room axis (depth [B,H,W], masks [B,n,H,W], labels [B,H,W]) and ``channels`` is one
    list of names per room; a room with fewer masks pads its list with ``None`` (the plane is not read).  ``channels`` may also be an
    int32 device tensor [B,n] of NYU class indices (< 0: padding), which costs no host work - the form to use under a graph capture.
    The result is the builder's static output buffer: the next call overwrites it.  The call allocates nothing, reads nothing back
    and runs on the current stream.

    If no depth value of a room lies below ``min + 20`` the reference raises (``np.max`` of an empty selection).  The kernel leaves 1
    in that room's word of ``status`` (int32 [B], device).  ``validate=True`` reads it after every call - one synchronisation - and
    raises ``ValueError``; the default does not read it, and such a room's depth channel is NaN."""

    def __init__(self, H, W, size=256, batch=1, device="cuda", validate=False):
        self.H, self.W, self.size, self.batch, self.validate = int(H), int(W), int(size), int(batch), validate
        self.device = torch.device(device)
        fh, wh = band_table(self.H, self.size)
        fw, ww = band_table(self.W, self.size)
        self.width_h, self.width_w = wh.shape[1], ww.shape[1]
        self._first_h, self._w_h = torch.from_numpy(fh).to(self.device), torch.from_numpy(wh).to(self.device)
        self._first_w = torch.from_numpy(fw).to(self.device)
        self._w_w = torch.from_numpy(np.ascontiguousarray(ww.T)).to(self.device)          # [width, size]: see sln_hip.h
        nbytes = L.lib().sln_spade_input_workspace_bytes(self.batch)
        if nbytes < 0:
            L.check(nbytes, "sln_spade_input_workspace_bytes")
        self._ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        self.out = torch.empty(self.batch, 41, self.size, self.size, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self._channels = {}

    def _channel_table(self, channels, n):
        if torch.is_tensor(channels):
            if channels.dtype != torch.int32 or channels.numel() != self.batch * n or channels.device != self.out.device:
                raise ValueError("channels: int32 [%d, %d] on %s expected" % (self.batch, n, self.out.device))
            return channels.contiguous()
        rows = [list(channels)] if self.batch == 1 and (len(channels) == 0 or channels[0] is None or isinstance(channels[0], str)) \
            else [list(c) for c in channels]
        if len(rows) != self.batch or any(len(r) != n for r in rows):
            raise ValueError("channels: %d list(s) of %d class names expected" % (self.batch, n))
        key = tuple(tuple(r) for r in rows)
        if key not in self._channels:
            idx = [[-1 if nm is None else NYU40.index(nm) for nm in r] for r in rows]
            for r in idx:
                live = [c for c in r if c >= 0]
                if len(set(live)) != len(live):
                    raise ValueError("channels: a class is named twice in one room")
            self._channels[key] = torch.tensor(idx, dtype=torch.int32).reshape(self.batch, n).to(self.device)
        return self._channels[key]

    def _room_array(self, t, what, dtypes, planes=False):
        if not torch.is_tensor(t) or t.device != self.out.device or t.dtype not in dtypes:
            raise ValueError("%s: a %s tensor on %s expected" % (what, " / ".join(str(d) for d in dtypes), self.out.device))
        tail = (self.H, self.W)
        if tuple(t.shape[-2:]) != tail or t.numel() % (self.batch * self.H * self.W) or (not planes and t.numel() != self.batch * self.H * self.W):
            raise ValueError("%s: shape %s does not hold %d room(s) of %d x %d" % (what, tuple(t.shape), self.batch, self.H, self.W))
        return t.contiguous()

    def __call__(self, depth, masks=None, channels=None, labels=None):
        depth = self._room_array(depth, "depth", (torch.float32,))
        chan, n_live = None, 0
        if labels is not None:
            if masks is not None or channels is not None:
                raise ValueError("give masks and channels, or labels")
            planes, mode = self._room_array(labels, "labels", (torch.uint8,)), 2
        elif masks is not None and masks.numel():
            planes = self._room_array(masks, "masks", (torch.uint8, torch.float32), planes=True)
            mode = 0 if planes.dtype == torch.uint8 else 1
            n_live = planes.numel() // (self.batch * self.H * self.W)
            if n_live > 40 or channels is None:
                raise ValueError("masks: at most 40 planes per room, with the class of each in `channels`")
            chan = self._channel_table(channels, n_live)
        else:
            planes, mode = None, 0
        L.check(L.lib().sln_spade_input_forward(L.ptr(depth), L.ptr(planes), mode, L.ptr(chan), n_live, self.batch, self.H, self.W, self.size,
                                                L.ptr(self._first_h), L.ptr(self._w_h), self.width_h, L.ptr(self._first_w), L.ptr(self._w_w),
                                                self.width_w, L.ptr(self._ws), L.ptr(self.out), L.ptr(self.status), L.current_stream_ptr()),
                "sln_spade_input_forward")
        torch.autograd.graph.increment_version(self.out)       # written through its pointer: SPADEGenerator4 keeps a map's planes by version
        if self.validate:
            bad = self.status.cpu().nonzero().flatten().tolist()
            if bad:
                raise ValueError("no depth value below min + 20 in room(s) %s: the reference's np.max of an empty selection" % bad)
        return self.out


def build_inputs(depths, masks_list, size=256):
    """depths: B tensors [H,W] on the device, masks_list: B dicts {class name: [H,W] mask, uint8 or float32} -> [B,41,size,size]"""
    B = len(depths)
    H, W = depths[0].shape
    dev = depths[0].device
    n = max([len(m) for m in masks_list] + [1])
    dtype = torch.uint8 if all(v.dtype == torch.uint8 for m in masks_list for v in m.values()) else torch.float32
    planes = torch.zeros(B, n, H, W, dtype=dtype, device=dev)
    names = []
    for b, m in enumerate(masks_list):
        for j, (name, v) in enumerate(m.items()):
            planes[b, j] = v.to(dev)
        names.append(list(m) + [None] * (n - len(m)))
    builder = InputBuilder(H, W, size=size, batch=B, device=dev)
    return builder(torch.stack([d.to(dev).float() for d in depths]), masks=planes, channels=names)


def colorize_rooms(model, builder, rooms, num_z, generator=None):
    """rooms: keyword dicts of ``builder`` (batch 1), e.g. {"depth": d, "masks": planes, "channels": names} or {"depth": d,
    "labels": l}, device tensors.  For each room: the input on the device and ONE ``colorize`` call.  -> uint8 [R, num_z, S, S, 3];
    nothing is read back in between."""
    if builder.batch != 1:
        raise ValueError("colorize_rooms shades one room per generator call: a batch-1 builder expected")
    return torch.stack([to_uint8(colorize(model, builder(**room), num_z, generator)) for room in rooms])
