"""The gradient of a view's intrinsics, restated (sln_place_camera_step_views, csrc/placement.hip; DESIGN §4 "Intrinsics of the target views").

project() forms ``u = xh K[0] + yh K[1] + K[2]``, ``v = os - (xh K[3] + yh K[4] + K[5])`` with ``xh = x / (z + proj_eps)``, ``yh = y / (z + proj_eps)``
and ndc ``= 2 (. - os / 2) / os``.  With ``s2 = 2 / os`` and ``(gu, gv)`` a corner's image gradient - the face's plus its fill_back copy's -

    dL/dfx = sum s2 gu xh,    dL/dfy = sum -s2 gv yh,    dL/dcx = sum s2 gu,    dL/dcy = sum -s2 gv

(``fx = K[0]``, ``fy = K[4]``, ``cx = K[2]``, ``cy = K[5]``) over the three corners of every face the view does not cull.

``intr_grad_ref`` works from the kernel's float32 operands - the face table, the PLACED corners (world space), the camera, grad_faces - and
evaluates every product in ``dtype`` in the kernel's order: ``su = s2 * gu``, ``sv = s2 * gv``, ``iz = 1 / (z + proj_eps)``, ``xh = x * iz``,
``yh = y * iz``, the terms ``su * xh``, ``-(sv * yh)``, ``su``, ``-sv``; the sums over the corners are float64 whatever ``dtype`` is, as the
kernel's are.  With ``dtype=np.float64`` it is the reference, with ``np.float32`` a model of the kernel's own rounding.

Allowance per element: ``(POSE_C + 0.5 sqrt(n)) 2^-24 S`` - the pose gradient's (tests/pose_refine_ref.py), whose chains are the longer
ones - with ``S = sum |term|`` over the float64 terms and ``n`` the number of corners summed.  A term here is at most: the camera
coordinate (3 products, 3 additions), z + proj_eps, the reciprocal, x * iz, gu = a + b, s2 (a quotient), s2 * gu and the last product: 12
roundings.  ``S`` takes the terms as they are, not the absolute-value form of what lies under them: a camera coordinate that cancels
against its translation is not allowed for; the float32 run of this file measures how much of the allowance that takes
(tests/test_intrinsics_refine_host.py holds it to half).
"""
import numpy as np

from pose_refine_ref import pose_bound as intr_bound      # the bound is the pose kernel's, constant included


def intr_grad_ref(faces, corners, K, R, t, grad_faces, orig_size, proj_eps, cull_eps, dtype=np.float64):
    """``faces`` [F, 3] int (into ``corners``), ``corners`` [Vtot, 3] float32 placed vertices, ``K``, ``R`` [3, 3], ``t`` [3] float32,
    ``grad_faces`` [>= 2F, 3, 3] float32 (rows F .. 2F - 1: the fill_back copies, corners (2, 1, 0)) ->
    (g [4] float64: d fx, d fy, d cx, d cy;  S [4] float64;  n: corners summed;  kept [F] bool).
    The cull is the kernel's float32 decision (``z < cull_eps`` in any corner) whatever ``dtype`` is."""
    f = dtype
    faces = np.asarray(faces).astype(np.int64)
    F = faces.shape[0]
    p32 = np.asarray(corners, dtype=np.float32)[faces]                                   # [F, 3 corners, 3]
    R32, t32 = (np.asarray(x, dtype=np.float32).reshape(-1) for x in (R, t))
    gf32 = np.asarray(grad_faces, dtype=np.float32)

    def camera(p, Rv, tv):
        return [p[..., 0] * Rv[3 * j] + p[..., 1] * Rv[3 * j + 1] + p[..., 2] * Rv[3 * j + 2] + tv[j] for j in range(3)]

    z32 = camera(p32, R32, t32)[2]
    kept = ~(z32 < np.float32(cull_eps)).any(1)
    p = p32[kept].astype(f)
    x, y, z = camera(p, R32.astype(f), t32.astype(f))
    a = gf32[:F][kept].astype(f)                                                         # [n, corner q, 3]
    b = gf32[F:2 * F][kept][:, ::-1].astype(f)                                           # the copy's corner 2 - q
    gu, gv = (a[..., j] + b[..., j] for j in range(2))
    s2 = f(2) / f(orig_size)
    su, sv = s2 * gu, s2 * gv
    iz = f(1) / (z + f(proj_eps))
    xh, yh = x * iz, y * iz
    terms = [(su * xh).astype(np.float64), (-(sv * yh)).astype(np.float64), su.astype(np.float64), (-sv).astype(np.float64)]
    g = np.array([float(v.sum()) for v in terms])
    S = np.array([float(np.abs(v).sum()) for v in terms])
    return g, S, 3 * int(kept.sum()), kept
