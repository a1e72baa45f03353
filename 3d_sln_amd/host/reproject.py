"""An observed depth and label frame of ANY pinhole camera -> the pair ``observe.ObservedTarget`` takes: ``depth`` [B, S, S] float32
and ``labels`` [B, S, S] uint8 as ``get_cam_mat``'s camera of the room row sees them, in the row order of the scene tensor's planes
(csrc/observed_reproject.hip; DESIGN §4 "Observed frames from any camera" is the definition).

The frame is a depth image seen as a mesh: every cell of four neighbouring pixels gives two triangles in the source camera, the pose
takes them to the target camera, ``sln_raster_forward`` draws them, and a compose step reads depth and the label of the nearest source
pixel out of the rasterizer's maps.

  * ``ObservedReprojector``   static buffers, three steps of launches (faces, raster, compose), nothing read back;
  * ``reproject_torch``       the definition in torch ops with the caller's rasterizer: the yardstick of the tests and the CPU route;
  * ``ObservedFuser``         V frames per room: faces and raster over R * V frames, then ONE fused compose (csrc/observed_fuse.hip) that
    gives every target pixel to the frame with the nearest surface there - the z-buffer rule - and says which frame won, how many
    frames saw the pixel and how many of them agree with the winner's depth; ``fuse_torch`` / ``reproject_views_torch`` restate it
    (DESIGN §4 "Several observed frames per room");
  * ``pose_step_torch``, ``rotation_exp``, ``pose_error``   the float64 restatement of a pose step of ``RefineBatch(poses=)`` and the
    distance of two poses (DESIGN §4 "Camera poses of the target views");
  * ``intrinsics_step_torch``, ``intrinsics_error``   the same for a step of ``RefineBatch(intrinsics=)`` on focal lengths and principal
    point (DESIGN §4 "Intrinsics of the target views");
  * ``relative_pose``, ``refine_view``, ``look_at_view``, ``scene_as_source``   the cameras: source -> target pose from two world poses,
    the refinement view of a room row, a further view of the room from an eye and a point it looks at (``RefineBatch(views=)``), and the
    source intrinsics under which a scene tensor's own planes are a frame of their own camera.

A target pixel no face covers - a disocclusion, a cut at a depth step, the frame's border - reads "no reading" (-1, label 0);
``RefineBatch(mask="readings")`` keeps such pixels out of the loss, and further frames of the room fill them (``ObservedFuser``).  A
frame finer than the target is decimated in front of the route by an integer factor (``prefilter=``, ``ObservedPrefilter``,
``prefilter_torch``, ``prefilter_factor``; csrc/observed_prefilter.hip; DESIGN §4 "Observed frames finer than the target"): depths and
labels of two surfaces are never blended, and V is ragged only by ``fx = 0`` padding.
"""
import numpy as np
import torch

from .. import _lib as L
from . import diff_render as DR
from .observe import FAR

PROJ_EPS = 1e-9
NO_READING = -1.0
MAX_FACES = 1 << 24
MAX_S = 4096
MAX_B = 65535
MAX_V = 255
MAX_PREFILTER = 8
# corner -> (row, column) offset inside the cell, per slot: (a, b, c) and (d, c, b)
_DI = ((0, 1, 0), (1, 0, 1))
_DJ = ((0, 0, 1), (1, 1, 0))


def n_faces(Hs, Ws):
    return 2 * (int(Hs) - 1) * (int(Ws) - 1)


def _reading(d32):
    """a float32 depth is a reading when 0 < d <= 15 (a NaN has none): csrc/observed_rules.h, obs_reading"""
    return (d32 > 0) & (d32 <= FAR)


def _check_sizes(B, Hs, Ws, S):
    """the limits of csrc/observed_rules.h for B frames as the face step sees them"""
    if B < 1 or B > MAX_B or Hs < 2 or Ws < 2 or S < 1 or S > MAX_S or n_faces(Hs, Ws) > MAX_FACES:
        raise ValueError("batch in [1, 65535], a frame of at least 2 x 2 pixels and at most 2^24 faces, S in [1, 4096] expected, got "
                         "batch = %r, Hs = %r, Ws = %r, S = %r" % (B, Hs, Ws, S))


def _check_views(R, V):
    if R < 1 or V < 1 or V > MAX_V:
        raise ValueError("rooms >= 1 and views in [1, 255] expected, got rooms = %r, views = %r" % (R, V))


def _check_scalars(orig_size, near, gap):
    if not orig_size > 0 or not gap >= 0 or not near > 0:
        raise ValueError("orig_size > 0, gap >= 0 and near > 0 expected, got %r, %r, %r" % (orig_size, gap, near))


def check_tensors(specs, device, contiguous=True, cuda=False):
    """``specs``: (tensor, dtype, shape, name) per argument.  Raises ValueError for what is no tensor of that dtype on ``device`` (with
    ``cuda``: on a GPU at all), or not of that shape (with ``contiguous``: and contiguous).  Reads nothing but the tensors' metadata."""
    for t, dt, shape, what in specs:
        if not torch.is_tensor(t) or t.dtype != dt or t.device != device or (cuda and not t.is_cuda):
            raise ValueError("%s: a %s tensor on %s expected" % (what, str(dt).replace("torch.", ""), device))
        if tuple(t.shape) != tuple(shape) or (contiguous and not t.is_contiguous()):
            raise ValueError("%s: shape %s is not %s%s" % (what, tuple(t.shape), "a contiguous " if contiguous else "", list(shape)))


# ------------------------------------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------------------------------------
def relative_pose(R_src, t_src, R_tgt, t_tgt):
    """World -> camera poses ``p = R w + t`` of the source and the target camera ([..., 3, 3] and [..., 3] or [..., 1, 3]) -> the pose
    [..., 3, 4] float32 that takes source-camera coordinates to target-camera coordinates, ``[R_t R_s^T | t_t - R_t R_s^T t_s]``,
    computed in float64 and rounded once."""
    Rs, Rt = torch.as_tensor(R_src).double(), torch.as_tensor(R_tgt).double()
    ts = torch.as_tensor(t_src).double().reshape(*Rs.shape[:-2], 3, 1)
    tt = torch.as_tensor(t_tgt).double().reshape(*Rt.shape[:-2], 3, 1)
    rel = torch.matmul(Rt, Rs.transpose(-1, -2))
    return torch.cat((rel, tt - torch.matmul(rel, ts)), -1).float().contiguous()


def refine_view(room_box, S):
    """The refinement view of a room row (``diff_render.get_cam_mat``): -> (K_tgt [3, 3], R [3, 3], t [3], orig_size) on the host.  K is
    in pixels of ``orig_size`` whatever the image size ``S`` of the render."""
    if int(S) < 1:
        raise ValueError("S: a positive image size expected")
    room = [float(x) for x in torch.as_tensor(room_box).detach().cpu().reshape(-1).tolist()]
    K, R, t = DR.get_cam_mat([room], "cpu")
    return K[0].contiguous(), R[0].contiguous(), t.reshape(3).contiguous(), float(DR.inter_out)


def look_at_view(eye, at):
    """A further view of a room in ``get_cam_mat``'s convention (``p_cam = R p_world + t``, ``K`` in pixels of ``diff_render.inter_out``): the
    camera at ``eye`` [3] looking at ``at`` [3], both in room coordinates (y up), without roll -> (K [3, 3], R [3, 3], t [3], orig_size) float32
    on the host - what ``refine_view`` returns for the refinement camera, and what ``RefineBatch(views=)`` takes per view.  ``K`` is
    ``get_cam_mat``'s; ``R = c2cv [right; up; back]`` with back = (eye - at) / |eye - at|, right = y x back normalised, up = back x right and
    the ``c2cv`` flip diag(1, -1, -1); ``t = -R eye``.  Computed in float64 and rounded once.  With ``get_cam_mat``'s eye and a point on its
    axis this is ``get_cam_mat``'s camera.  Refused: non-finite input, ``eye == at``, a view straight up or down (no roll is defined)."""
    e, a = (torch.as_tensor(x).detach().cpu().double().reshape(-1) for x in (eye, at))
    if e.numel() != 3 or a.numel() != 3 or not (torch.isfinite(e).all() and torch.isfinite(a).all()):
        raise ValueError("look_at_view: eye and at are finite points [3]")
    back = e - a
    if not float(back.norm()) > 0:
        raise ValueError("look_at_view: eye and at coincide")
    back = back / back.norm()
    right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), back)
    if not float(right.norm()) > 1e-9:
        raise ValueError("look_at_view: a view along the y axis has no roll-free orientation")
    right = right / right.norm()
    up = torch.linalg.cross(back, right)
    R = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64)) @ torch.stack((right, up, back))
    K = DR.get_cam_mat([[0.0] * 6], "cpu")[0][0]
    return K.contiguous(), R.float().contiguous(), (-(R @ e)).float().contiguous(), float(DR.inter_out)


SMALL_ANGLE = 1e-8       # below it exp([w]x) is evaluated by its series (csrc/placement.hip, place_pose_step_views_kernel)


def _skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack((torch.stack((z, -w[..., 2], w[..., 1]), -1), torch.stack((w[..., 2], z, -w[..., 0]), -1),
                        torch.stack((-w[..., 1], w[..., 0], z), -1)), -2)


def rotation_exp(omega, series=None):
    """``exp([omega]x)`` [..., 3, 3] in float64: ``I + A W + B W^2`` with ``A = sin(th) / th``, ``B = 2 sin^2(th / 2) / th^2`` (Rodrigues), and
    below ``|omega| = 1e-8`` their series ``A = 1 - th^2 / 6``, ``B = 1 / 2 - th^2 / 24``.  ``series``: None (by the angle), True or False
    (one branch everywhere: for comparing the two)."""
    w = torch.as_tensor(omega).double()
    th2 = (w * w).sum(-1)
    th = th2.sqrt()
    small = (th < SMALL_ANGLE) if series is None else torch.full_like(th, bool(series), dtype=torch.bool)
    safe = torch.where(th > 0, th, torch.ones_like(th))
    A = torch.where(small, 1.0 - th2 / 6.0, torch.sin(safe) / safe)
    B = torch.where(small, 0.5 - th2 / 24.0, 2.0 * torch.sin(0.5 * safe) ** 2 / (safe * safe))
    W = _skew(w)
    eye = torch.eye(3, dtype=torch.float64, device=w.device).expand_as(W)
    return eye + A[..., None, None] * W + B[..., None, None] * torch.matmul(W, W)


def pose_step_torch(Rm, t, omega, tau):
    """One pose step in float64 (DESIGN §4 "Camera poses of the target views"): the rigid motion ``p_cam' = exp([omega]x) p_cam + tau``
    applied in the camera frame of ``p_cam = Rm p_world + t``:  ``Rm <- E Rm``, ``t <- E t + tau``.  ``Rm`` [..., 3, 3], ``t``, ``omega``,
    ``tau`` [..., 3] -> (Rm, t) float64.  The restatement of the update of sln_place_pose_step_views."""
    Rm, t, tau = (torch.as_tensor(x).double() for x in (Rm, t, tau))
    E = rotation_exp(omega)
    return torch.matmul(E, Rm), torch.matmul(E, t[..., None])[..., 0] + tau


def pose_error(Rm_a, t_a, Rm_b, t_b):
    """-> (angle of ``Rm_a Rm_b^T`` in radians, distance of the two camera centres ``-Rm^T t``), float64, per leading index"""
    Ra, ta, Rb, tb = (torch.as_tensor(x).double() for x in (Rm_a, t_a, Rm_b, t_b))
    rel = (Ra[..., :, None, :] * Rb[..., None, :, :]).sum(-1)          # Ra Rb^T, symmetric by bits for Ra == Rb: a pose against itself gives 0
    cos = (rel.diagonal(dim1=-2, dim2=-1).sum(-1) - 1.0) / 2.0
    sin = torch.stack((rel[..., 2, 1] - rel[..., 1, 2], rel[..., 0, 2] - rel[..., 2, 0], rel[..., 1, 0] - rel[..., 0, 1]), -1).norm(dim=-1) / 2.0
    ca = -torch.matmul(Ra.transpose(-1, -2), ta[..., None])[..., 0]
    cb = -torch.matmul(Rb.transpose(-1, -2), tb[..., None])[..., 0]
    return torch.atan2(sin, cos), (ca - cb).norm(dim=-1)


FOCAL_LOG_MAX = 1.0      # SLN_FOCAL_LOG_MAX of include/sln_hip.h: one step scales a focal length by e^-1 .. e at the most


def intrinsics_step_torch(K, grad, focal_step, center_step, tie_focal=True):
    """One intrinsics step in float64 (DESIGN §4 "Intrinsics of the target views"): ``K`` [..., 3, 3], ``grad`` [..., 4] = (dL/dfx, dL/dfy,
    dL/dcx, dL/dcy) -> K float64 with  ``fx <- fx exp(sx)``, ``fy <- fy exp(sy)``,  ``sx = -focal_step fx dL/dfx``, ``sy = -focal_step fy dL/dfy``
    or, tied, the one log-scale ``sx = sy = -focal_step (fx dL/dfx + fy dL/dfy)`` - each held to ``[-FOCAL_LOG_MAX, FOCAL_LOG_MAX]``, so that
    a focal length stays positive and finite whatever the gradient - and ``cx <- cx - center_step dL/dcx``, ``cy`` likewise (pixels of
    ``orig_size``).  Every other entry of ``K`` is returned as it came.  The restatement of the update of sln_place_camera_step_views."""
    K, g = torch.as_tensor(K).double().clone(), torch.as_tensor(grad).double()
    fs, cs = float(focal_step), float(center_step)
    fx, fy = K[..., 0, 0].clone(), K[..., 1, 1].clone()
    sx, sy = -fs * (fx * g[..., 0]), -fs * (fy * g[..., 1])
    if tie_focal:
        sx = sy = -fs * (fx * g[..., 0] + fy * g[..., 1])
    sx, sy = sx.clamp(-FOCAL_LOG_MAX, FOCAL_LOG_MAX), sy.clamp(-FOCAL_LOG_MAX, FOCAL_LOG_MAX)
    K[..., 0, 0], K[..., 1, 1] = fx * torch.exp(sx), fy * torch.exp(sy)
    K[..., 0, 2], K[..., 1, 2] = K[..., 0, 2] - cs * g[..., 2], K[..., 1, 2] - cs * g[..., 3]
    return K


def intrinsics_move(p_cam, leaf, fx, fy, proj_eps=1e-9):
    """The camera-space points ``p_cam`` [..., 3] moved so that an UNCHANGED zero-skew ``K`` with focal lengths ``fx``, ``fy`` projects them where
    ``K`` with ``fx e^sx, fy e^sy, cx + dcx, cy + dcy`` would project ``p_cam``; ``leaf`` = (sx, sy, dcx, dcy):  ``x' = e^sx x + dcx (z +
    proj_eps) / fx``, ``y'`` likewise, ``z`` as it is (``proj_eps``: the projection's ``xh = x / (z + proj_eps)``).  Differentiable in ``leaf``:
    its gradient at 0 is ``(fx dL/dfx, fy dL/dfy, dL/dcx, dL/dcy)`` - how ``finetune_vae(intrinsics=)`` reaches K through a renderer that
    takes it as a constant."""
    zz = p_cam[..., 2] + proj_eps
    return torch.stack((torch.exp(leaf[0]) * p_cam[..., 0] + leaf[2] * zz / fx, torch.exp(leaf[1]) * p_cam[..., 1] + leaf[3] * zz / fy,
                        p_cam[..., 2]), -1)


def intrinsics_error(K_a, K_b):
    """-> (relative focal error ``max(|fx_a - fx_b| / fx_b, |fy_a - fy_b| / fy_b)``, distance of the principal points in pixels), float64,
    per leading index; ``K_b`` is the reference"""
    Ka, Kb = torch.as_tensor(K_a).double(), torch.as_tensor(K_b).double()
    rel = torch.maximum((Ka[..., 0, 0] - Kb[..., 0, 0]).abs() / Kb[..., 0, 0], (Ka[..., 1, 1] - Kb[..., 1, 1]).abs() / Kb[..., 1, 1])
    return rel, torch.stack((Ka[..., 0, 2] - Kb[..., 0, 2], Ka[..., 1, 2] - Kb[..., 1, 2]), -1).norm(dim=-1)


def scene_as_source(K_tgt, orig_size, S):
    """The ``k_src`` [..., 4] (fx, fy, cx, cy) under which the planes of a scene tensor rendered at ``S`` with ``K_tgt`` [..., 3, 3] and
    ``orig_size`` are a source frame of that same camera, with the identity pose: plane row r, column c is the rasterizer's pixel
    (S - 1 - r, c), whose centre projects from ``K (x / z, y / z, 1) = orig_size / S * (c + 0.5, r + 0.5)`` - an ordinary x-right,
    y-down image of ``K * S / orig_size`` (no axis is mirrored; K's skew entry must be 0)."""
    K = torch.as_tensor(K_tgt).double()
    s = float(S) / float(orig_size)
    return (torch.stack((K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]), -1) * s).float().contiguous()


def prefilter_factor(k_src, K_tgt, orig_size, S, fmax=MAX_PREFILTER):
    """The largest decimation factor at which a coarse source pixel still subtends no more than a target pixel on the optical axis:
    ``floor(min over frames of min(fx, fy) * orig_size / (S * max over rooms of max(K00, K11)))`` in float64, clamped to [1, fmax].
    ``k_src`` [..., 4] (frames with fx <= 0 are padding and skipped), ``K_tgt`` [..., 3, 3].  The pose is not looked at: a camera much
    nearer to a surface than the target view sees it finer still, and the caller may pass a larger factor."""
    if not orig_size > 0 or int(S) < 1 or int(fmax) < 1 or int(fmax) > MAX_PREFILTER:
        raise ValueError("orig_size > 0, S >= 1 and fmax in [1, %d] expected, got %r, %r, %r" % (MAX_PREFILTER, orig_size, S, fmax))
    k = torch.as_tensor(k_src).detach().double().cpu().reshape(-1, 4)
    K = torch.as_tensor(K_tgt).detach().double().cpu().reshape(-1, 3, 3)
    k = k[k[:, 0] > 0]
    if k.shape[0] == 0:
        return 1
    src = float(torch.minimum(k[:, 0], k[:, 1]).min())
    tgt = float(torch.maximum(K[:, 0, 0], K[:, 1, 1]).max())
    ratio = src * float(orig_size) / (float(int(S)) * tgt)
    if not ratio >= 1.0:                                             # (a NaN, a coarser frame, a focal length that is not positive)
        return 1
    return int(min(float(int(fmax)), np.floor(ratio)))


def _check_prefilter(f, Hs, Ws, gap=0.0):
    if int(f) != f or f < 1 or f > MAX_PREFILTER or Hs < f or Ws < f or not gap >= 0:
        raise ValueError("an integer factor in [1, %d], a frame of at least f x f pixels and gap >= 0 expected, got f = %r, Hs = %r, Ws = %r, "
                         "gap = %r" % (MAX_PREFILTER, f, Hs, Ws, gap))


# ------------------------------------------------------------------------------------------------------------------------------
# the definition in torch ops
# ------------------------------------------------------------------------------------------------------------------------------
def prefilter_torch(depth_src, labels_src, k_src, f, gap=0.05):
    """csrc/observed_prefilter.hip in torch ops on the tensors' device (DESIGN §4 "Observed frames finer than the target"):
    ``depth_src`` [B, Hs, Ws] float, ``labels_src`` [B, Hs, Ws] uint8, ``k_src`` [B, 4] -> (depth [B, Hs // f, Ws // f] float32, labels
    uint8, k_out [B, 4] float32, counts [B, 3] int64: coarse pixels whose block is all members, with a reading but fewer members,
    without a reading)."""
    if depth_src.dim() != 3 or labels_src.shape != depth_src.shape or labels_src.dtype != torch.uint8 or tuple(k_src.shape) != (depth_src.shape[0], 4):
        raise ValueError("depth_src [B, Hs, Ws] float, labels_src [B, Hs, Ws] uint8 and k_src [B, 4] expected")
    B, Hs, Ws = depth_src.shape
    _check_prefilter(f, Hs, Ws, gap)
    f = int(f)
    Hd, Wd, n = Hs // f, Ws // f, f * f
    dev = depth_src.device
    blocks = lambda t: t[:, :f * Hd, :f * Wd].reshape(B, Hd, f, Wd, f).permute(0, 1, 3, 2, 4).reshape(B, Hd, Wd, n)   # row-major inside the block
    d, lab = blocks(depth_src.float()), blocks(labels_src).long()
    reading = _reading(d)
    r = reading.sum(-1)
    has = 2 * r >= n
    inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    ranked = torch.sort(torch.where(reading, d, inf), -1).values                                  # the readings in ascending order, then inf
    dref = torch.gather(ranked, -1, ((r - 1).clamp(min=0) // 2)[..., None])                       # the lower median
    hi, lo = torch.maximum(d, dref), torch.minimum(d, dref)
    member = reading & ~((hi - lo) > torch.tensor(gap, dtype=torch.float32, device=dev) * lo)      # float32, the face kernel's test
    m = member.sum(-1)
    total = torch.zeros(B, Hd, Wd, dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for t in range(n):                                               # row-major order of the block, one rounded addition each
        total = total + torch.where(member[..., t], 1.0 / d[..., t].double(), zero)
    depth = torch.where(has, (m.double() / total).float(), torch.zeros((), dtype=torch.float32, device=dev))
    votes = torch.zeros(B, Hd, Wd, n, dtype=torch.long, device=dev)
    for u in range(n):                                               # votes[t]: the members that carry pixel t's byte
        votes += (member[..., u, None] & (lab[..., u, None] == lab)).long()
    key = torch.where(member, votes * 256 + (255 - lab), torch.full((), -1, dtype=torch.long, device=dev))    # most votes, then the smallest byte
    labels = torch.where(has, 255 - key.max(-1).values % 256, torch.zeros((), dtype=torch.long, device=dev)).to(torch.uint8)
    counts = torch.stack(((has & (m == n)).sum(dim=(1, 2)), (has & (m < n)).sum(dim=(1, 2)), (~has).sum(dim=(1, 2))), 1)
    k_out = k_src.float() / torch.tensor(float(f), dtype=torch.float32, device=k_src.device)
    return depth.contiguous(), labels.contiguous(), k_out.contiguous(), counts


def faces_torch(depth_src, k_src, pose, K_tgt, orig_size, near=0.1, gap=0.05, dtype=torch.float64):
    """csrc/observed_reproject.hip's first kernel in torch ops, in ``dtype``: -> faces_xyz [B, F, 3, 3].  The two decisions on the
    source depths (reading, depth step) are float32 operations in either precision: they are part of the definition."""
    _check_scalars(orig_size, near, gap)
    d32 = depth_src.float()
    B, Hs, Ws = d32.shape
    dev = d32.device
    reading = _reading(d32)
    d = d32.to(dtype)
    k, P, K = k_src.to(dtype), pose.to(dtype), K_tgt.to(dtype)
    fx, fy, cx, cy = (k[:, e, None, None] for e in range(4))
    u = (torch.arange(Ws, device=dev).to(dtype) + 0.5)[None, None, :]
    v = (torch.arange(Hs, device=dev).to(dtype) + 0.5)[None, :, None]
    xs, ys = (u - cx) / fx * d, (v - cy) / fy * d
    cam = [(xs * P[:, i, 0, None, None] + ys * P[:, i, 1, None, None]) + d * P[:, i, 2, None, None] + P[:, i, 3, None, None] for i in range(3)]
    os_ = float(orig_size)
    xh, yh = cam[0] / (cam[2] + PROJ_EPS), cam[1] / (cam[2] + PROJ_EPS)
    uu = (xh * K[:, 0, 0, None, None] + yh * K[:, 0, 1, None, None]) + K[:, 0, 2, None, None]
    vv = os_ - ((xh * K[:, 1, 0, None, None] + yh * K[:, 1, 1, None, None]) + K[:, 1, 2, None, None])
    vert = torch.stack((2.0 * (uu - os_ / 2.0) / os_, 2.0 * (vv - os_ / 2.0) / os_, cam[2]), -1)          # [B, Hs, Ws, 3]

    def cell(t):
        a, b, c, dd = t[:, :-1, :-1], t[:, 1:, :-1], t[:, :-1, 1:], t[:, 1:, 1:]
        return torch.stack((torch.stack((a, b, c), 3), torch.stack((dd, c, b), 3)), 3)                     # [B, Hs-1, Ws-1, 2, 3, ...]
    faces = cell(vert)
    ok = cell(reading).all(-1)
    dc = cell(torch.where(reading, d32, torch.ones_like(d32)))
    dmin, dmax = dc.min(-1).values, dc.max(-1).values
    step = (dmax - dmin) > torch.tensor(gap, dtype=torch.float32, device=dev) * dmin
    behind = ~(faces[..., 2] >= near).all(-1)
    frame_ok = ((k_src[:, 0] > 0) & (k_src[:, 1] > 0))[:, None, None, None]
    cull = ~ok | step | behind | ~frame_ok
    faces = torch.where(cull[..., None, None], torch.zeros_like(faces), faces)
    return faces.reshape(B, n_faces(Hs, Ws), 3, 3).contiguous()


def _hit_and_label(face_index, weight, labels_src):
    """compose's rule per frame, in raster order: -> hit [B, S, S] bool (``face_index`` in [0, F), no NaN among the three weights) and
    the byte of ``labels_src`` at the face's corner of largest weight, ties to the lower corner number ([B, S, S] uint8; meaningless
    where there is no hit)"""
    B, Hs, Ws = labels_src.shape
    Wc, F = Ws - 1, n_faces(Hs, Ws)
    dev = face_index.device
    fi = face_index.long()
    w = weight.float()
    hit = (fi >= 0) & (fi < F) & ~torch.isnan(w).any(-1)
    k = fi.clamp(0, F - 1)
    cell, which = k // 2, k % 2
    ci, cj = cell // Wc, cell % Wc
    first = w[..., 1] > w[..., 0]
    corner = first.long()
    corner = torch.where(w[..., 2] > torch.where(first, w[..., 1], w[..., 0]), torch.full_like(corner, 2), corner)
    di, dj = torch.tensor(_DI, device=dev)[which, corner], torch.tensor(_DJ, device=dev)[which, corner]
    frame = torch.arange(B, device=dev)[:, None, None]
    return hit, labels_src[frame, ci + di, cj + dj]


def compose_torch(face_index, weight, raster_depth, labels_src):
    """csrc/observed_reproject.hip's compose in torch ops: maps [B, S, S] in raster order and ``labels_src`` [B, Hs, Ws] uint8 ->
    (depth [B, S, S] float32, labels [B, S, S] uint8) in the planes' row order, hits [B] int64"""
    dev = face_index.device
    hit, lab = _hit_and_label(face_index, weight, labels_src)
    labels = torch.where(hit, lab, torch.zeros((), dtype=torch.uint8, device=dev))
    depth = torch.where(hit, raster_depth.float(), torch.full((), NO_READING, dtype=torch.float32, device=dev))
    return torch.flip(depth, [1]).contiguous(), torch.flip(labels, [1]).contiguous(), hit.sum(dim=(1, 2))


def fuse_torch(face_index, weight, raster_depth, labels_src, V, gap=0.05):
    """The fusion of V frames per room in torch ops (DESIGN §4 "Several observed frames per room"): the rasterizer's maps [R * V, S, S(, 3)]
    in raster order, frame ``r * V + v``, and ``labels_src`` [R * V, Hs, Ws] uint8 -> dict, in the planes' row order:

      depth  [R, S, S] float32  the depth of the WINNER: of the contributing frames (a hit by compose's rule whose depth is no NaN) the one
                                with the smallest depth, equal depths to the lowest v; -1 where no frame contributes
      labels [R, S, S] uint8    the winner's label by compose's rule (a 0 of the winner stays 0); 0 without a winner
      source [R, S, S] uint8    1 + v of the winner, 0 without one
      count  [R, S, S] uint8    contributing frames
      agree  [R, S, S] uint8    contributing frames with ``!((d_v - dmin) > gap * dmin)`` in float32 (the winner among them)
      hits [R], wins [R, V] int64   pixels with a winner, pixels per winning frame"""
    B, Hs, Ws = labels_src.shape
    V = int(V)
    if V < 1 or V > MAX_V or B % V or not gap >= 0:
        raise ValueError("V in [1, 255] that divides the %d frames and gap >= 0 expected, got V = %r, gap = %r" % (B, V, gap))
    R, S = B // V, int(face_index.shape[1])
    dev = face_index.device
    hit, lab = _hit_and_label(face_index, weight, labels_src)
    d = raster_depth.float().reshape(R, V, S, S)
    contributes = (hit.reshape(R, V, S, S) & ~torch.isnan(d))
    lab = lab.reshape(R, V, S, S)
    best = torch.full((R, S, S), -1, dtype=torch.long, device=dev)
    dmin = torch.full((R, S, S), NO_READING, dtype=torch.float32, device=dev)
    labels = torch.zeros((R, S, S), dtype=torch.uint8, device=dev)
    for v in range(V):                                               # v upwards, a strict <: the z-buffer rule
        take = contributes[:, v] & ((best < 0) | (d[:, v] < dmin))
        dmin = torch.where(take, d[:, v], dmin)
        labels = torch.where(take, lab[:, v], labels)
        best = torch.where(take, torch.full_like(best, v), best)
    edge = torch.tensor(gap, dtype=torch.float32, device=dev) * dmin  # one float32 product ...
    near = ~((d - dmin[:, None]) > edge[:, None])                     # ... against one float32 difference
    count = contributes.sum(1)
    agree = (contributes & near).sum(1)
    wins = torch.stack([(best == v).sum(dim=(1, 2)) for v in range(V)], 1)
    flip = lambda x, dt: torch.flip(x, [1]).to(dt).contiguous()
    return dict(depth=flip(dmin, torch.float32), labels=flip(labels, torch.uint8), source=flip(best + 1, torch.uint8),
                count=flip(count, torch.uint8), agree=flip(agree, torch.uint8), hits=(best >= 0).sum(dim=(1, 2)), wins=wins)


def _route_torch(depth_src, labels_src, k_src, pose, K_tgt, orig_size, S, rasterize, near, far, gap, dtype, prefilter):
    """What the two torch routes share, over B frames [B, Hs, Ws] with a ``K_tgt`` each: the filter (not run at ``prefilter`` 1:
    non-readings pass to the face step as they are), ``faces_torch``, the caller's rasterizer and the way back from numpy -> (the
    labels the last step gathers from, faces_xyz, face_index, weight, raster_depth)"""
    _check_prefilter(prefilter, *depth_src.shape[-2:])
    if int(prefilter) > 1:
        depth_src, labels_src, k_src = prefilter_torch(depth_src, labels_src, k_src, prefilter, gap)[:3]
    B, Hs, Ws = depth_src.shape
    _check_sizes(B, Hs, Ws, int(S))
    fxyz = faces_torch(depth_src, k_src, pose, K_tgt, orig_size, near, gap, dtype)
    maps = rasterize(fxyz.float().cpu().numpy(), int(S), float(near), float(far))
    fi, w, dep = (torch.from_numpy(np.ascontiguousarray(x)).to(depth_src.device) for x in maps)
    return labels_src, fxyz, fi, w, dep


def reproject_torch(depth_src, labels_src, k_src, pose, K_tgt, orig_size, S, rasterize, near=0.1, far=100.0, gap=0.05, dtype=torch.float64,
                    prefilter=1):
    """The route of ``ObservedReprojector`` in torch ops on the tensors' device, in ``dtype``.  ``rasterize(faces float32 numpy
    [B, F, 3, 3], image_size, near, far) -> (face_index, weight, depth)`` numpy maps in raster order is the caller's rasterizer (the
    tests pass the C restatement the rasterizer kernels are held to).  -> dict(depth [B, S, S] float32, labels [B, S, S] uint8,
    hits [B] int64, faces_xyz [B, F, 3, 3] in ``dtype``, face_index, weight).  With ``prefilter`` f > 1 the frames go through
    ``prefilter_torch`` first and everything else runs on the coarse frames: F is that of Hs // f x Ws // f."""
    if depth_src.dim() != 3 or labels_src.shape != depth_src.shape or labels_src.dtype != torch.uint8:
        raise ValueError("depth_src [B, Hs, Ws] float and labels_src [B, Hs, Ws] uint8 expected")
    lab, fxyz, fi, w, dep = _route_torch(depth_src, labels_src, k_src, pose, K_tgt, orig_size, S, rasterize, near, far, gap, dtype, prefilter)
    depth, labels, hits = compose_torch(fi, w, dep, lab)
    return dict(depth=depth, labels=labels, hits=hits, faces_xyz=fxyz, face_index=fi, weight=w)


def reproject_views_torch(depth_src, labels_src, k_src, pose, K_tgt, orig_size, S, rasterize, near=0.1, far=100.0, gap=0.05,
                          dtype=torch.float64, prefilter=1):
    """The route of ``ObservedFuser`` in torch ops on the tensors' device, in ``dtype``: ``reproject_torch``'s counterpart for V frames
    per room.  ``depth_src`` [R, V, Hs, Ws] float, ``labels_src`` [R, V, Hs, Ws] uint8, ``k_src`` [R, V, 4], ``pose`` [R, V, 3, 4],
    ``K_tgt`` [R, 3, 3] (the room's); ``rasterize`` as in ``reproject_torch``.  -> the dict of ``fuse_torch`` plus faces_xyz
    [R * V, F, 3, 3] in ``dtype`` and the maps face_index, weight, raster_depth [R * V, S, S(, 3)].  ``prefilter`` as in
    ``reproject_torch``."""
    if depth_src.dim() != 4 or labels_src.shape != depth_src.shape or labels_src.dtype != torch.uint8:
        raise ValueError("depth_src [R, V, Hs, Ws] float and labels_src [R, V, Hs, Ws] uint8 expected")
    R, V = depth_src.shape[:2]
    if tuple(k_src.shape) != (R, V, 4) or tuple(pose.shape) != (R, V, 3, 4) or tuple(K_tgt.shape) != (R, 3, 3):
        raise ValueError("k_src [R, V, 4], pose [R, V, 3, 4] and K_tgt [R, 3, 3] expected")
    _check_views(R, V)
    B, frame = R * V, depth_src.shape[2:]
    lab, fxyz, fi, w, dep = _route_torch(depth_src.reshape(B, *frame), labels_src.reshape(B, *frame), k_src.reshape(B, 4), pose.reshape(B, 3, 4),
                                         K_tgt.repeat_interleave(V, 0), orig_size, S, rasterize, near, far, gap, dtype, prefilter)
    out = fuse_torch(fi, w, dep, lab, V, gap)
    out.update(faces_xyz=fxyz, face_index=fi, weight=w, raster_depth=dep)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the device route
# ------------------------------------------------------------------------------------------------------------------------------
def _stream(out):
    """the current stream of a device buffer; host tensors (the argument checks' tests: refused before any launch) have none"""
    return L.current_stream_ptr() if out.is_cuda else None


def faces(depth_src, k_src, pose, K_tgt, orig_size, near, gap, faces_xyz):
    """the bare launch of ``sln_reproject_faces`` over the caller's buffers (contiguous float32 on the device)"""
    d = L.SlnReproject()
    d.depth_src, d.k_src, d.pose, d.K_tgt = depth_src.data_ptr(), k_src.data_ptr(), pose.data_ptr(), K_tgt.data_ptr()
    d.B, d.Hs, d.Ws = (int(x) for x in depth_src.shape)
    d.orig_size, d.near, d.gap = float(orig_size), float(near), float(gap)
    L.check(L.lib().sln_reproject_faces(d, L.ptr(faces_xyz), _stream(faces_xyz)), "sln_reproject_faces")


def compose(face_index, weight, raster_depth, labels_src, depth_out, labels_out, hits):
    """the bare ``sln_reproject_compose`` call over the caller's buffers"""
    B, Hs, Ws = (int(x) for x in labels_src.shape)
    L.check(L.lib().sln_reproject_compose(L.ptr(face_index), L.ptr(weight), L.ptr(raster_depth), L.ptr(labels_src), B, Hs, Ws,
                                          int(face_index.shape[1]), L.ptr(depth_out), L.ptr(labels_out), L.ptr(hits), _stream(depth_out)),
            "sln_reproject_compose")


def prefilter(depth_src, labels_src, k_src, f, gap, depth_out, labels_out, k_out, counts=None):
    """the bare ``sln_observed_prefilter`` call over the caller's buffers (contiguous, on the device); ``counts`` [B, 3] int64 is optional"""
    B, Hs, Ws = (int(x) for x in depth_src.shape)
    L.check(L.lib().sln_observed_prefilter(L.ptr(depth_src), L.ptr(labels_src), L.ptr(k_src), B, Hs, Ws, int(f), float(gap), L.ptr(depth_out),
                                           L.ptr(labels_out), L.ptr(k_out), L.ptr(counts), _stream(depth_out)), "sln_observed_prefilter")


def _device(who, device, torch_name):
    """the device of ``who``'s static buffers: a CUDA device, ``cuda`` normalised to the current index (what a tensor's ``.device`` says)"""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.SlnError("%s runs on the MI355X only (no CPU fallback); %s restates it for CPU tensors" % (type(who).__name__, torch_name))
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _frame_specs(lead, Hs, Ws, depth_src, labels_src, k_src):
    """``check_tensors``' specs of the per-frame inputs; ``lead`` is (B,) or (R, V)"""
    return [(depth_src, torch.float32, lead + (Hs, Ws), "depth_src"), (labels_src, torch.uint8, lead + (Hs, Ws), "labels_src"),
            (k_src, torch.float32, lead + (4,), "k_src")]


class ObservedPrefilter:
    """``batch`` frames of ``Hs`` x ``Ws`` decimated by the integer factor ``f`` on the device, in front of the reprojection (DESIGN §4
    "Observed frames finer than the target"; ``prefilter_factor`` chooses ``f``).

        pf = ObservedPrefilter(480, 640, 2, batch=16)
        depth, labels, k_out = pf(depth_src, labels_src, k_src)          # [16, 240, 320], [16, 240, 320], [16, 4]

    A coarse pixel takes the harmonic mean of the readings of its f x f block that lie on the surface of the block's lower median
    depth, and those readings' most frequent label; it has no reading (0.0, label 0) when fewer than half the block's pixels have one.
    ``counts`` [B, 3] int64 (blocks that are all one surface, blocks with a reading otherwise, blocks without) is an attribute.  The
    outputs are the instance's static buffers.  A call is two launches on the current stream, allocates nothing and reads nothing
    back: legal under a graph capture.  Tensors of another dtype, device or shape are refused before anything is launched."""

    def __init__(self, Hs, Ws, f, batch=1, gap=0.05, device="cuda"):
        self.Hs, self.Ws, self.batch, self.gap = int(Hs), int(Ws), int(batch), float(gap)
        _check_prefilter(f, self.Hs, self.Ws, self.gap)
        self.f = int(f)
        if self.batch < 1 or self.batch > MAX_B:
            raise ValueError("batch in [1, 65535] expected, got %r" % (batch,))
        B, dev = self.batch, _device(self, device, "prefilter_torch")
        self.device, self.Hd, self.Wd = dev, self.Hs // self.f, self.Ws // self.f
        self.depth = torch.empty(B, self.Hd, self.Wd, dtype=torch.float32, device=dev)
        self.labels = torch.empty(B, self.Hd, self.Wd, dtype=torch.uint8, device=dev)
        self.k_out = torch.empty(B, 4, dtype=torch.float32, device=dev)
        self.counts = torch.zeros(B, 3, dtype=torch.int64, device=dev)

    def check(self, depth_src, labels_src, k_src):
        """raises ValueError before anything is launched; reads the instance's sizes and device only"""
        check_tensors(_frame_specs((self.batch,), self.Hs, self.Ws, depth_src, labels_src, k_src), self.device)

    def __call__(self, depth_src, labels_src, k_src):
        self.check(depth_src, labels_src, k_src)
        prefilter(depth_src, labels_src, k_src, self.f, self.gap, self.depth, self.labels, self.k_out, self.counts)
        return self.depth, self.labels, self.k_out


class _ObservedRoute:
    """What ``ObservedReprojector`` and ``ObservedFuser`` share: ``batch`` frames of ``Hs`` x ``Ws`` through (the filter,) the face step and
    the rasterizer into maps of ``S`` x ``S``.  Owns the size and scalar checks, the device, ``pre`` (the ``ObservedPrefilter``, or None),
    ``Hd`` x ``Wd`` (the frames the face step sees), ``F`` and the buffers faces_xyz, face_index, weight, raster_depth; a subclass adds
    its outputs and its last step."""

    def __init__(self, torch_name, Hs, Ws, S, batch, near, far, gap, device, prefilter):
        self.Hs, self.Ws, self.S, self.batch = int(Hs), int(Ws), int(S), int(batch)
        self.near, self.far, self.gap = float(near), float(far), float(gap)
        _check_prefilter(prefilter, self.Hs, self.Ws)
        self.prefilter = int(prefilter)
        self.Hd, self.Wd = self.Hs // self.prefilter, self.Ws // self.prefilter
        _check_sizes(self.batch, self.Hd, self.Wd, self.S)
        _check_scalars(1.0, self.near, self.gap)
        self.device = dev = _device(self, device, torch_name)
        B, S = self.batch, self.S
        self.pre = ObservedPrefilter(self.Hs, self.Ws, self.prefilter, B, self.gap, dev) if self.prefilter > 1 else None
        self.F = n_faces(self.Hd, self.Wd)
        self.faces_xyz = torch.zeros(B, self.F, 3, 3, dtype=torch.float32, device=dev)
        self.face_index = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        self.weight = torch.empty(B, S, S, 3, dtype=torch.float32, device=dev)
        self.raster_depth = torch.empty(B, S, S, dtype=torch.float32, device=dev)
        self._raster_ws = torch.empty(int(L.lib().sln_raster_workspace_bytes(B, self.F)), dtype=torch.uint8, device=dev)

    def raster(self):
        """``sln_raster_forward`` over ``faces_xyz`` into the maps, on the current stream"""
        L.check(L.lib().sln_raster_forward(L.ptr(self.faces_xyz), self.batch, self.F, self.S, self.near, self.far, L.ptr(self._raster_ws),
                                           L.ptr(self.face_index), L.ptr(self.weight), L.ptr(self.raster_depth), L.current_stream_ptr()),
                "sln_raster_forward")

    def _maps(self, depth_src, labels_src, k_src, pose, K_tgt, orig_size):
        """(filter,) faces and raster over the ``batch`` flat frames; -> the labels the last step gathers from"""
        if self.pre is not None:
            depth_src, labels_src, k_src = self.pre(depth_src, labels_src, k_src)
        faces(depth_src, k_src, pose, K_tgt, orig_size, self.near, self.gap, self.faces_xyz)
        self.raster()
        return labels_src


def _check_route(me, lead, depth_src, labels_src, k_src, pose, K_tgt, orig_size):
    """the ``check`` of both routes: raises ValueError before anything is launched; reads ``me``'s sizes, scalars and device only.
    ``lead`` is (B,) or (R, V): the leading sizes of the per-frame tensors, whose first is that of ``K_tgt``"""
    check_tensors(_frame_specs(lead, me.Hs, me.Ws, depth_src, labels_src, k_src) +
                  [(pose, torch.float32, lead + (3, 4), "pose"), (K_tgt, torch.float32, lead[:1] + (3, 3), "K_tgt")], me.device)
    _check_scalars(float(orig_size), me.near, me.gap)


class ObservedReprojector(_ObservedRoute):
    """Frames of ``batch`` rooms, each ``Hs`` x ``Ws``, brought into target views of ``S`` x ``S`` on the device.

        rp = ObservedReprojector(480, 640, 256, batch=16)
        depth, labels, hits = rp(depth_src, labels_src, k_src, pose, K_tgt, orig_size)
        rb = RefineBatch(model, rooms, observed=(depth, labels), image_size=256, ...)

    ``depth_src`` [B, Hs, Ws] float32 (metric, along the optical axis; a reading when 0 < d <= 15), ``labels_src`` [B, Hs, Ws] uint8
    (0 none, 1 + c NYU class c; any byte passes through), ``k_src`` [B, 4] float32 (fx, fy, cx, cy in source pixels; a frame whose
    focal lengths are not positive yields nothing), ``pose`` [B, 3, 4] float32 (source camera -> target camera: ``relative_pose``),
    ``K_tgt`` [B, 3, 3] float32 and ``orig_size`` (``refine_view``).  -> ``depth`` [B, S, S] float32 (-1 where no face was hit),
    ``labels`` [B, S, S] uint8, ``hits`` [B] int64 (hit pixels per frame).  These are the instance's static buffers: the next call
    overwrites them.  A call makes three steps of launches (faces, raster, compose) on the current stream, allocates nothing and reads
    nothing back: legal under a graph capture.  Tensors of another dtype, device or shape are refused before anything is launched.

    ``prefilter`` f > 1 (``prefilter_factor``) puts an ``ObservedPrefilter`` in front, as ``self.pre``: the three steps then run on
    frames of ``Hs // f`` x ``Ws // f`` (at least 2 x 2) with f * f times fewer faces, and ``labels`` are gathered from the coarse
    labels.  With 1, the default, the filter is not run."""

    def __init__(self, Hs, Ws, S, batch=1, near=0.1, far=100.0, gap=0.05, device="cuda", prefilter=1):
        super().__init__("reproject_torch", Hs, Ws, S, batch, near, far, gap, device, prefilter)
        B, S, dev = self.batch, self.S, self.device
        self.depth = torch.empty(B, S, S, dtype=torch.float32, device=dev)
        self.labels = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
        self.hits = torch.zeros(B, dtype=torch.int64, device=dev)

    def check(self, depth_src, labels_src, k_src, pose, K_tgt, orig_size):
        _check_route(self, (self.batch,), depth_src, labels_src, k_src, pose, K_tgt, orig_size)

    def __call__(self, depth_src, labels_src, k_src, pose, K_tgt, orig_size):
        self.check(depth_src, labels_src, k_src, pose, K_tgt, orig_size)
        lab = self._maps(depth_src, labels_src, k_src, pose, K_tgt, orig_size)
        compose(self.face_index, self.weight, self.raster_depth, lab, self.depth, self.labels, self.hits)
        return self.depth, self.labels, self.hits


def fuse(face_index, weight, raster_depth, labels_src, V, gap, depth_out, labels_out, hits, source_out=None, count_out=None, agree_out=None,
         wins=None):
    """the bare ``sln_reproject_fuse`` call over the caller's buffers (maps and ``labels_src`` of R * V frames); the last four are optional"""
    B, Hs, Ws = (int(x) for x in labels_src.shape)
    V = int(V)
    if V < 1 or B % V:
        raise ValueError("V >= 1 that divides the %d frames expected, got %r" % (B, V))
    L.check(L.lib().sln_reproject_fuse(L.ptr(face_index), L.ptr(weight), L.ptr(raster_depth), L.ptr(labels_src), B // V, V, Hs, Ws,
                                       int(face_index.shape[1]), float(gap), L.ptr(depth_out), L.ptr(labels_out), L.ptr(source_out),
                                       L.ptr(count_out), L.ptr(agree_out), L.ptr(hits), L.ptr(wins), _stream(depth_out)),
            "sln_reproject_fuse")


def confidence_from_agree(agree, full, out, work):
    """``agree`` uint8 (frames within ``gap`` of the winner's depth, the winner included; 0 without a winner) -> ``out`` uint8, the confidence
    byte ``(min(agree, full) * 255 + full // 2) // full``: 0 without a winner, 255 from ``full`` agreeing frames on (128 for one frame at
    ``full`` = 2).  ``work``: an int32 tensor of ``agree``'s shape.  Integer ops in place: allocates nothing."""
    full = int(full)
    if full < 1 or full > 255:
        raise ValueError("confidence: full is a frame count in [1, 255], got %r" % (full,))
    work.copy_(agree)
    work.clamp_(max=full).mul_(255).add_(full // 2)
    torch.div(work, full, rounding_mode="floor", out=work)
    return out.copy_(work)


class ObservedFuser(_ObservedRoute):
    """``views`` frames per room of ``rooms`` rooms, each ``Hs`` x ``Ws``, fused into one target view of ``S`` x ``S`` per room on the
    device: where several frames see a target pixel, the one with the nearest surface there has it (the z-buffer rule).

        fu = ObservedFuser(480, 640, 256, rooms=16, views=4)
        depth, labels, source = fu(depth_src, labels_src, k_src, pose, K_tgt, orig_size)
        rb = RefineBatch(model, rooms, observed=(depth, labels), mask=fu.valid(), image_size=256, ...)      # or mask="readings"
        corroborated = (fu.agree >= 2).to(torch.uint8)          # pixels two frames agree on, for mask= - built by the caller
        rb = RefineBatch(model, rooms, observed=(depth, labels), confidence=fu.confidence(), ...)      # graded: seen once counts half

    ``depth_src`` [R, V, Hs, Ws] float32, ``labels_src`` [R, V, Hs, Ws] uint8, ``k_src`` [R, V, 4] float32, ``pose`` [R, V, 3, 4] float32
    - per frame, as ``ObservedReprojector`` takes them; a room with fewer frames pads with frames whose ``k_src`` has fx = 0 -, ``K_tgt``
    [R, 3, 3] float32 and ``orig_size`` per room (``refine_view``).  -> ``depth`` [R, S, S] float32 (-1 without a winner), ``labels``
    [R, S, S] uint8, ``source`` [R, S, S] uint8 (1 + v of the winning frame, 0 without one); ``count``, ``agree`` [R, S, S] uint8
    (frames that see the pixel; those within ``gap`` of the winner's depth, itself included), ``hits`` [R] and ``wins`` [R, V] int64
    are attributes.  All are the instance's static buffers: the next call overwrites them.  A call spreads ``K_tgt`` over the frames
    with one ``copy_`` and makes three steps of launches (faces and raster over R * V frames, the fused compose) on the current stream,
    allocates nothing and reads nothing back: legal under a graph capture.  Tensors of another dtype, device or shape are refused
    before anything is launched.  ``prefilter`` f > 1 as in ``ObservedReprojector``: one ``ObservedPrefilter`` over the R * V frames
    (``self.pre``) in front, everything else on frames of ``Hs // f`` x ``Ws // f``."""

    def __init__(self, Hs, Ws, S, rooms=1, views=1, near=0.1, far=100.0, gap=0.05, device="cuda", prefilter=1):
        R, V = self.rooms, self.views = int(rooms), int(views)
        _check_views(R, V)
        super().__init__("reproject_views_torch", Hs, Ws, S, R * V, near, far, gap, device, prefilter)
        S, dev = self.S, self.device
        self.K_frames = torch.zeros(R * V, 3, 3, dtype=torch.float32, device=dev)
        self.depth = torch.empty(R, S, S, dtype=torch.float32, device=dev)
        self.labels, self.source, self.count, self.agree, self._valid = (torch.empty(R, S, S, dtype=torch.uint8, device=dev) for _ in range(5))
        self.hits = torch.zeros(R, dtype=torch.int64, device=dev)
        self.wins = torch.zeros(R, V, dtype=torch.int64, device=dev)
        self._conf, self._conf_work = torch.empty(R, S, S, dtype=torch.uint8, device=dev), torch.empty(R, S, S, dtype=torch.int32, device=dev)

    def check(self, depth_src, labels_src, k_src, pose, K_tgt, orig_size):
        """raises ValueError before anything is launched; reads the instance's sizes, scalars and device only"""
        _check_route(self, (self.rooms, self.views), depth_src, labels_src, k_src, pose, K_tgt, orig_size)

    def __call__(self, depth_src, labels_src, k_src, pose, K_tgt, orig_size):
        self.check(depth_src, labels_src, k_src, pose, K_tgt, orig_size)
        R, V, B = self.rooms, self.views, self.batch
        self.K_frames.view(R, V, 3, 3).copy_(K_tgt[:, None])
        lab = self._maps(depth_src.view(B, self.Hs, self.Ws), labels_src.view(B, self.Hs, self.Ws), k_src.view(B, 4), pose.view(B, 3, 4),
                         self.K_frames, orig_size)
        fuse(self.face_index, self.weight, self.raster_depth, lab, V, self.gap, self.depth, self.labels, self.hits, self.source, self.count,
             self.agree, self.wins)
        return self.depth, self.labels, self.source

    def valid(self):
        """``source > 0`` as uint8 [R, S, S] in a static buffer: the tensor ``RefineBatch(mask=)`` takes (no allocation, nothing read back)"""
        return self._valid.copy_(self.source).clamp_(max=1)

    def confidence(self, full=2):
        """``(min(agree, full) * 255 + full // 2) // full`` as uint8 [R, S, S] in a static buffer: the tensor ``RefineBatch(confidence=)`` takes
        - 0 without a winner, 128 for a pixel one frame saw, 255 from ``full`` frames that agree on (no allocation, nothing read back).
        ``full`` outside [1, 255] is refused, and so is a fuser without the ``agree`` plane."""
        if getattr(self, "agree", None) is None:
            raise ValueError("confidence: this fuser was built without the agree plane")
        return confidence_from_agree(self.agree, full, self._conf, self._conf_work)
