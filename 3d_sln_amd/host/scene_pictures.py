"""The pictures of the refinement loop on the device: what ``testing/test_render_refine.py`` writes with ``save_images`` (:144-163, called
for the target :320 and for iterations 0 and 59 :377) and ``save_label_depth`` (:118-142), from a scene tensor [B, 70 | 41, S, S] that
stays where the renderer left it (csrc/scene_pictures.hip, three launches):

  * ``depth8``  [B, S, S] uint8      ``d = x - min``; ``m = max(d[d < 10])``; ``d[d > 10] = m``; ``(d / m * 255).astype(uint8)`` (:149-156)
  * ``labels``  [B, S, S] uint8      the two statements :343-344 at full resolution: ``1 + argmax`` over the 40 semantic planes, ``0`` where
    their sum is below 0.5 (the reference's ``-100``) - the class-index image ``spade_input.InputBuilder(labels=...)`` takes
  * ``rgb``     [B, S, S, 3] uint8   ``CLASS_COLORS[labels]``: ``save_label_depth``'s picture, black where empty (:123-132)
  * ``masks8``  [B, 40, S, S] uint8  ``(255 * plane).astype(uint8)`` (:159-162)
  * ``status``  [B] int32            bit 0: no ``d < 10`` (the reference's ``np.max`` raises), bit 1: ``m == 0`` (it divides by zero); the
    room's depth bytes are 0 then.  ``d == 10`` exactly is outside the reference's defined behaviour (its uint8 cast overflows): 255.

``ScenePictures`` owns static buffers like ``spade_input.InputBuilder``; ``scene_pictures_torch`` restates the kernels in torch ops on any
device (float32, the same order of operations) - the tests and tools/scene_pictures_time.py hold the kernels to it; ``save_images`` /
``save_label_depth`` keep the reference's call shape.
"""
import collections
import os
import warnings

import torch

from .. import _lib as L
from . import plot2d as _P
from .spade_input import NYU40

# test_render_refine.py:34-76 (mapped_colors): entry 0 is "no class", entry 1 + c the colour of NYU class c - plot2d's table behind a black
CLASS_COLORS = ((0, 0, 0),) + tuple(_P.MAPPED_COLORS)
# :32 (nyu_class): the names its file names carry - with blanks where spade_input.NYU40 (mask FILE names) has underscores
NYU_CLASS = tuple(n.replace("_", " ") for n in NYU40)
FAR = 10.0
N_SEM = 40

Pictures = collections.namedtuple("Pictures", "depth8 labels rgb masks8 status")


def palette_tensor(device=None):
    """[41] int32 (the bits of r | g << 8 | b << 16)"""
    return torch.tensor([_P.pack_rgb(c) for c in CLASS_COLORS], dtype=torch.int32, device=device)


def clean_image(image, live):
    """``image`` with the planes ``live`` [B, C] (SlnRefineLoss::live_planes) flags dead as zeros and those flagged 1 as ones"""
    if live is None:
        return image
    f = live.to(image.device).to(torch.int32)[:, :, None, None]
    out = torch.where((f & 1) == 0, torch.zeros_like(image), image)
    return torch.where(f == 1, torch.ones_like(image), out)


def scene_pictures_torch(image, live=None, masks=True):
    """``image`` [B, C >= 41, S, S] float32 on any device -> ``Pictures`` (masks8 None without ``masks``): the restatement of
    csrc/scene_pictures.hip in torch ops, batched over the rooms, nothing read back."""
    x = clean_image(image.float(), live)
    B = x.shape[0]
    d = x[:, 0] - x[:, 0].amin(dim=(1, 2), keepdim=True)
    neg = torch.full_like(d, float("-inf"))
    m = torch.where(d < FAR, d, neg).amax(dim=(1, 2), keepdim=True)
    none, flat = m == float("-inf"), m == 0
    d = torch.where(d > FAR, m.expand_as(d), d)
    v = (d / m) * 255.0
    v = torch.where(none | flat, torch.zeros_like(v), torch.nan_to_num(v, nan=0.0).clamp(0.0, 255.0))
    depth8 = v.to(torch.uint8)
    status = (none.reshape(B).to(torch.int32) | (flat.reshape(B).to(torch.int32) << 1))
    sem = x[:, 1:1 + N_SEM]
    arg = torch.argmax(sem, dim=1)
    labels = torch.where(sem.sum(dim=1) < 0.5, torch.zeros_like(arg), arg + 1).to(torch.uint8)
    pal = palette_tensor(x.device).to(torch.int64)[labels.to(torch.int64)]
    rgb = torch.stack([pal & 255, (pal >> 8) & 255, (pal >> 16) & 255], -1).to(torch.uint8)
    masks8 = (255.0 * sem).clamp(0.0, 255.0).to(torch.uint8) if masks else None
    return Pictures(depth8, labels, rgb, masks8, status)


def _check_geometry(S, batch, channels):
    if int(S) < 4 or int(S) % 4 != 0 or int(S) > 32768:
        raise ValueError("S must be a positive multiple of 4 (four pixels a lane), got %r" % (S,))
    if int(batch) < 1 or int(batch) > 65535:
        raise ValueError("batch must be in [1, 65535], got %r" % (batch,))
    if int(channels) not in (41, 70):
        raise ValueError("channels must be 70 (a scene tensor) or 41 (depth + the 40 semantic planes), got %r" % (channels,))


class ScenePictures:
    """``Pictures`` of ``batch`` rooms [batch, channels, S, S] float32 on the device (csrc/scene_pictures.hip).

        pics = ScenePictures(256, batch=16)
        depth8, labels, rgb, masks8, status = pics(rb.image, live=rb.live)

    ``live`` [batch, channels] uint8 are the plane flags the sparse scene pass leaves (``RefineBatch.live``): dead planes are not read.
    ``masks=False`` (default) leaves ``masks8`` None and uncomputed - it is two thirds of the bytes written.  The results are the
    instance's static buffers: the next call overwrites them.  A call allocates nothing, reads nothing back and runs on the current
    stream (three launches; legal under a graph capture).  Tensors that are not float32, not on the device or of another shape are
    refused before anything is launched."""

    def __init__(self, S, batch=1, channels=70, masks=False, device="cuda"):
        _check_geometry(S, batch, channels)
        self.S, self.batch, self.channels = int(S), int(batch), int(channels)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.SlnError("ScenePictures runs on the MI355X only (no CPU fallback); scene_pictures_torch restates it for CPU tensors")
        nbytes = L.lib().sln_scene_pictures_workspace_bytes(self.batch, self.S)
        if nbytes < 0:
            L.check(nbytes, "sln_scene_pictures_workspace_bytes")
        B, S = self.batch, self.S
        u8 = dict(dtype=torch.uint8, device=self.device)
        self._ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        self._palette = palette_tensor(self.device)
        self.depth8, self.labels, self.rgb = torch.empty(B, S, S, **u8), torch.empty(B, S, S, **u8), torch.empty(B, S, S, 3, **u8)
        self.masks8 = torch.empty(B, N_SEM, S, S, **u8) if masks else None
        self.status = torch.zeros(B, dtype=torch.int32, device=self.device)

    def check(self, image, live=None):
        if not torch.is_tensor(image) or image.dtype != torch.float32 or image.device.type != "cuda" or image.device != self.depth8.device:
            raise ValueError("image: a float32 tensor on %s expected" % self.depth8.device)
        if tuple(image.shape) != (self.batch, self.channels, self.S, self.S):
            raise ValueError("image: shape %s is not [%d, %d, %d, %d]" % (tuple(image.shape), self.batch, self.channels, self.S, self.S))
        if live is not None and (not torch.is_tensor(live) or live.dtype != torch.uint8 or live.device != image.device or
                                 tuple(live.shape) != (self.batch, self.channels)):
            raise ValueError("live: a uint8 tensor [%d, %d] on %s expected" % (self.batch, self.channels, image.device))

    def into(self, image, live, depth8, labels=None, rgb=None, masks8=None, status=None):
        """the three launches with the caller's output buffers (contiguous uint8 of the shapes above; None: not computed)"""
        self.check(image, live)
        image = image.contiguous()
        L.check(L.lib().sln_scene_pictures(L.ptr(image), self.batch, self.channels, self.S, L.ptr(None if live is None else live.contiguous()),
                                           L.ptr(self._palette), L.ptr(self._ws), L.ptr(depth8), L.ptr(labels), L.ptr(rgb), L.ptr(masks8),
                                           L.ptr(self.status if status is None else status), L.current_stream_ptr()), "sln_scene_pictures")

    def __call__(self, image, live=None):
        self.into(image, live, self.depth8, self.labels, self.rgb, self.masks8)
        return Pictures(self.depth8, self.labels, self.rgb, self.masks8, self.status)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's call shapes
# ------------------------------------------------------------------------------------------------------------------------------
def _to_device(t):
    t = torch.as_tensor(t).detach()
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            raise L.SlnError("the pictures are drawn on the MI355X only (no CPU fallback) and no device is visible")
        t = t.cuda()
    return t.float().contiguous()


def _write(array, path):
    try:
        from PIL import Image
    except ImportError:
        warnings.warn("scene_pictures: PIL is not installed, %r was not written" % (path,))
        return None
    Image.fromarray(array.cpu().numpy()).save(path, format="PNG")
    return path


def _folder(folder_name):
    if not os.path.isdir(folder_name):
        os.mkdir(folder_name)


def save_images(data, save_semantic=False, folder_name='./images', prefix='target'):
    """test_render_refine.py::save_images (:144-163) for ``data[0]`` of a scene tensor [N, 70 | 41, S, S] on the CPU or the device:
    ``<prefix>_depth.png`` and, with ``save_semantic``, ``<prefix>_<nyu class>.png`` for the 40 semantic planes (the reference writes
    ``.gif`` through imageio; on a 70-channel tensor its loop runs on to channel 41 and raises IndexError at ``nyu_class[40]`` - here the
    40 masks are written and the depth-hot planes left alone).  Files need PIL (a warning otherwise).  -> ``Pictures`` of the room."""
    _folder(folder_name)
    image = _to_device(data[0:1])
    pics = ScenePictures(image.shape[-1], 1, image.shape[1], masks=save_semantic, device=image.device)(image)
    _write(pics.depth8[0], os.path.join(folder_name, prefix + "_depth.png"))
    if save_semantic:
        for c, name in enumerate(NYU_CLASS):
            _write(pics.masks8[0, c], os.path.join(folder_name, prefix + "_{}.png".format(name)))
    return pics


def save_label_depth(data, depth_data, folder_name='./images', prefix='target'):
    """test_render_refine.py::save_label_depth (:118-142): ``data[0][0]`` [S, S] holds a class index 0..39 per pixel (below -1: empty,
    :343-344's -100), ``depth_data[0][0]`` the depth -> ``<prefix>_class_color.png`` and ``<prefix>_depth.png``.  The label map enters the
    kernel as the one-hot 41-channel tensor it stands for.  The reference hard-codes a 256 x 256 canvas; any S % 4 == 0 is taken.
    -> ``Pictures`` of the room."""
    _folder(folder_name)
    lab, depth = _to_device(data[0][0]), _to_device(depth_data[0][0])
    S = depth.shape[-1]
    cls = torch.round(lab)
    hit = torch.isclose(lab, cls) & (cls >= 0) & (cls < N_SEM)                      # np.isclose(image, i - 1), i = 1..40
    image = torch.zeros(1, 1 + N_SEM, S, S, device=depth.device)
    image[0, 0] = depth
    image[0, 1:].scatter_(0, cls.clamp(0, N_SEM - 1).to(torch.int64)[None], hit.float()[None])
    pics = ScenePictures(S, 1, 1 + N_SEM, device=depth.device)(image)
    _write(pics.rgb[0], os.path.join(folder_name, prefix + "_class_color.png"))
    _write(pics.depth8[0], os.path.join(folder_name, prefix + "_depth.png"))
    return pics
