"""Refinement targets from OBSERVED images: a metric depth image and a class-index image of the refinement camera -> the 70-plane
tensor ``refine.RefineLoss`` consumes - what ``RefineScene.render`` composes from its own rasterisation of ground-truth boxes, for a
room nobody has boxes of (csrc/observed_target.hip, two launches).

  * ``depth``   [B, S, S] float32  metric depth (plane 0 of a scene tensor); a pixel has a READING when ``0 < d <= 15`` - a NaN, an
    infinity, a value <= 0 and a value > 15 are none and become -1, the renderer's background value
  * ``labels``  [B, S, S] uint8    0 = no class, 1 + c = NYU class c (``scene_pictures`` labels, ``spade_input.InputBuilder(labels=)``);
    a byte > 40 and a byte on a pixel without a reading count as 0
  * ``target``  [B, 70, S, S]      plane 0 the cleaned depth, planes 1..40 the one-hot labels (exactly 0.0 / 1.0), planes 41.. the
    depth-hot planes of the class tables: ``d / wall_max`` inside a class's mask, ``mean_c / wall_max`` outside, with the scene pass's
    statistics (pixel count, 2^-32 fixed-point depth sum, the wall's maximum depth, 10 without a wall) and its float32 expressions
  * ``status``  [B] int32          bit 0: a byte > 40; bit 1: a label whose NYU channel no class of the tables has; bit 2: no wall
    pixel; bit 3: a byte in 1..40 on a pixel without a reading

Both images are in the row order of the scene tensor's planes.  ``ObservedTarget`` owns static buffers like
``scene_pictures.ScenePictures``; ``observed_target_torch`` is the same definition in torch ops on any device - the yardstick of the
tests and the CPU route; ``observe`` goes the other way (scene tensor -> depth, labels).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from . import scene_pictures as SP

N_SEM = 40
DEP0 = 41
FAR = 15.0
EMPTY_WALL_MAX = 10.0
STATUS_BAD_BYTE, STATUS_UNKNOWN_CLASS, STATUS_NO_WALL, STATUS_NO_READING = 1, 2, 4, 8


def _tables(chan, dch, nch):
    """host int32 arrays of the class tables, checked as the entry point checks them"""
    chan = np.ascontiguousarray(torch.as_tensor(chan).detach().cpu().numpy().astype(np.int32).reshape(-1))
    dch = np.ascontiguousarray(torch.as_tensor(dch).detach().cpu().numpy().astype(np.int32).reshape(-1))
    if chan.size != dch.size or not 1 <= chan.size <= 64:
        raise ValueError("chan and dch: 1..64 classes, one entry each")
    owned = dch[dch >= 0]
    if nch != DEP0 + owned.size or nch > 72:
        raise ValueError("nch = %d, the tables own %d depth-hot channels: nch must be 41 + that, at most 72" % (nch, owned.size))
    if chan.min() < 0 or chan.max() >= N_SEM or dch.min() < -1 or dch.max() >= nch - DEP0 or len(set(owned.tolist())) != owned.size:
        raise ValueError("chan must lie in [0, 40), dch in [-1, nch - 41), and no depth channel may be owned twice")
    return chan, dch


def observed_target_torch(depth, labels, chan, dch, nch=70):
    """``depth`` [B, S, S] float, ``labels`` [B, S, S] uint8 on any device -> (target [B, nch, S, S] float32, status [B] int32): the
    definition of csrc/observed_target.hip in torch ops, the int64 fixed-point sum included; nothing is read back."""
    chan, dch = _tables(chan, dch, nch)
    if depth.dim() != 3 or labels.shape != depth.shape or labels.dtype != torch.uint8:
        raise ValueError("depth [B, S, S] float32 and labels [B, S, S] uint8 expected")
    d = depth.float()
    dev = d.device
    B = d.shape[0]
    reading = (d > 0) & (d <= FAR)
    d0 = torch.where(reading, d, torch.full_like(d, -1.0))
    raw = labels.to(torch.int64)
    lab = torch.where((raw <= N_SEM) & reading, raw, torch.zeros_like(raw))
    out = torch.zeros(B, nch, *d.shape[1:], dtype=torch.float32, device=dev)
    out[:, 0] = d0
    out[:, 1:DEP0] = (lab[:, None] == torch.arange(1, N_SEM + 1, device=dev)[None, :, None, None]).float()
    fixed = torch.round(d0.double() * 4294967296.0).to(torch.int64)
    wall = lab == int(chan[0]) + 1
    wall_cnt = wall.sum(dim=(1, 2))
    wall_max = torch.where(wall, d0, torch.full_like(d0, float("-inf"))).amax(dim=(1, 2))
    wall_max = torch.where(wall_cnt > 0, wall_max, torch.full_like(wall_max, EMPTY_WALL_MAX))[:, None, None]
    for c in range(chan.size):
        if dch[c] < 0:
            continue
        mask = lab == int(chan[c]) + 1
        cnt = mask.sum(dim=(1, 2))
        total = (fixed * mask).sum(dim=(1, 2)).double() * (1.0 / 4294967296.0)
        mean = (total / cnt.double()).float()                                      # (0 / 0 where the class is absent: replaced below)
        fill = torch.where(cnt > 0, mean, wall_max[:, 0, 0])[:, None, None]
        out[:, DEP0 + int(dch[c])] = torch.where(mask, d0 / wall_max, (fill / wall_max).expand_as(d0))
    known = torch.zeros(N_SEM + 1, dtype=torch.bool)
    known[torch.from_numpy(chan.astype(np.int64)) + 1] = True
    named = (raw >= 1) & (raw <= N_SEM)
    bits = [(raw > N_SEM), (lab > 0) & ~known.to(dev)[lab], None, named & ~reading]
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    for k, hit in enumerate(bits):
        flag = (wall_cnt == 0) if hit is None else hit.reshape(B, -1).any(dim=1)
        status |= flag.to(torch.int32) << k
    return out, status


class ObservedTarget:
    """Targets of ``batch`` observed rooms on the device (csrc/observed_target.hip).

        ot = ObservedTarget(scene.chan, scene.dch, 256, batch=16)
        target, status = ot(depth, labels)              # [16, 70, 256, 256] float32, [16] int32

    ``chan`` / ``dch`` are the class tables of the rooms' scenes (``RefineScene.chan`` / ``.dch``: tensors on any device, or
    sequences); they are copied to the host once, here.  The results are the instance's static buffers: the next call overwrites them.
    A call allocates nothing, reads nothing back and runs on the current stream (two launches; legal under a graph capture).
    Tensors of another dtype, device or shape are refused before anything is launched."""

    def __init__(self, chan, dch, S, batch=1, device="cuda", nch=70):
        self.S, self.batch, self.nch = int(S), int(batch), int(nch)
        self.chan, self.dch = _tables(chan, dch, self.nch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SlnError("ObservedTarget runs on the MI355X only (no CPU fallback); observed_target_torch restates it for CPU tensors")
        nbytes = L.lib().sln_observed_target_workspace_bytes(self.batch, self.S)
        if nbytes < 0:
            raise ValueError("S must be a multiple of 4 in [4, 4096] and batch in [1, 65535], got S = %r, batch = %r" % (S, batch))
        self._ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=self.device)
        self.target = torch.empty(self.batch, self.nch, self.S, self.S, dtype=torch.float32, device=self.device)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=self.device)

    @staticmethod
    def check_tensors(depth, labels, shape, device):
        """``depth`` float32 and ``labels`` uint8, both of ``shape`` = (batch, S, S) on the CUDA ``device`` (a tensor's ``.device``)"""
        from .reproject import check_tensors                    # (reproject imports this module: FAR)
        check_tensors(((depth, torch.float32, shape, "depth"), (labels, torch.uint8, shape, "labels")), device, contiguous=False, cuda=True)

    def check(self, depth, labels):
        self.check_tensors(depth, labels, (self.batch, self.S, self.S), self.target.device)

    def into(self, depth, labels, target, status):
        """the two launches with the caller's output buffers (contiguous, [batch, nch, S, S] float32 and [batch] int32)"""
        self.check(depth, labels)
        depth, labels = depth.contiguous(), labels.contiguous()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(L.lib().sln_observed_target(L.ptr(depth), L.ptr(labels), self.batch, self.S, int(self.chan.size), vp(self.chan), vp(self.dch),
                                            self.nch, L.ptr(self._ws), L.ptr(target), L.ptr(status), L.current_stream_ptr()),
                "sln_observed_target")

    def __call__(self, depth, labels):
        self.into(depth, labels, self.target, self.status)
        return self.target, self.status


def observe(image, pictures=None):
    """A scene tensor [B, 70 | 41, S, S] -> (depth [B, S, S] float32, labels [B, S, S] uint8): plane 0 and the ``scene_pictures`` labels
    of a render made elsewhere in the library, in the planes' row order - an observation of that render.  Device tensors go through
    ``pictures`` (a ``scene_pictures.ScenePictures`` of the tensor's geometry; None: one is built for the call), host tensors through
    ``scene_pictures_torch``.  Both results are fresh tensors."""
    if not torch.is_tensor(image) or image.dim() != 4 or image.shape[1] < DEP0:
        raise ValueError("image: a scene tensor [B, 70 | 41, S, S] expected")
    image = image.detach().float()
    depth = image[:, 0].contiguous().clone()
    if image.device.type != "cuda":
        return depth, SP.scene_pictures_torch(image, masks=False).labels.contiguous()
    if pictures is None:
        pictures = SP.ScenePictures(image.shape[-1], batch=image.shape[0], channels=image.shape[1], device=image.device)
    return depth, pictures(image.contiguous()).labels.clone()
