"""The gradient of a view's pose, restated (sln_place_pose_step_views, csrc/placement.hip; DESIGN §4 "Camera poses of the target views").

Camera ``p_cam = R p_world + t``; a pose step is the rigid motion ``p_cam' = exp([w]x) p_cam + tau`` of the camera frame.  At w = tau = 0

    dL/dtau = sum g_cam,        dL/dw = sum p_cam x g_cam

over the three corners of every face the view does not cull, with ``g_cam = (gxh iz, gyh iz, gz - (gxh x + gyh y) iz^2)`` the camera-space
adjoint of a corner: face_adjoint()'s statements in their order, before its multiplication by R; the corner's image-plane gradient is the
sum of the face's and its fill_back copy's.

``pose_grad_ref`` works from the kernel's float32 operands - the face table, the PLACED corners (world space), the camera, grad_faces - and
evaluates every product in ``dtype`` in the kernel's order; the sums over the corners are float64 whatever ``dtype`` is, as the kernel's
are.  With ``dtype=np.float64`` it is the reference, with ``np.float32`` a model of the kernel's own rounding.

Allowance per element: ``(POSE_C + 0.5 sqrt(n)) 2^-24 S`` - the form and the constant of the projection adjoint's test
(tests/raster_bwd_gpu_util.py, PROJ_C: the longest rounding chain of a term, each rounding relative to the absolute-value form of what
lies under it), with ``S`` the sum over the corners of the absolute-value form of every product that enters the element and ``n`` the
number of corners summed.  The chain of gzc is that test's (33 roundings); the cross product multiplies it by a camera coordinate (6 + 1)
where the projection adjoint multiplies by an entry of R and adds twice (1 + 2): the float32 run of this file measures how much of the
allowance the longer chain takes (tests/test_pose_refine_host.py holds it to half; LAB_NOTES has the ratios).
"""
import numpy as np

U = 2.0 ** -24
POSE_C = 36.0


def pose_bound(S, n):
    return (POSE_C + 0.5 * np.sqrt(np.asarray(n, dtype=np.float64))) * U * S


def pose_grad_ref(faces, corners, K, R, t, grad_faces, orig_size, proj_eps, cull_eps, dtype=np.float64):
    """``faces`` [F, 3] int (into ``corners``), ``corners`` [Vtot, 3] float32 placed vertices, ``K``, ``R`` [3, 3], ``t`` [3] float32,
    ``grad_faces`` [>= 2F, 3, 3] float32 (rows F .. 2F - 1: the fill_back copies, corners (2, 1, 0)) ->
    (g [6] float64: d omega, d tau;  S [6] float64;  n: corners summed;  kept [F] bool).
    The cull is the kernel's float32 decision (``z < cull_eps`` in any corner) whatever ``dtype`` is."""
    f = dtype
    faces = np.asarray(faces).astype(np.int64)
    F = faces.shape[0]
    p32 = np.asarray(corners, dtype=np.float32)[faces]                                   # [F, 3 corners, 3]
    K32, R32, t32 = (np.asarray(x, dtype=np.float32).reshape(-1) for x in (K, R, t))
    gf32 = np.asarray(grad_faces, dtype=np.float32)

    def camera(p, Rv, tv):
        return [p[..., 0] * Rv[3 * j] + p[..., 1] * Rv[3 * j + 1] + p[..., 2] * Rv[3 * j + 2] + tv[j] for j in range(3)]

    z32 = camera(p32, R32, t32)[2]
    kept = ~(z32 < np.float32(cull_eps)).any(1)
    p = p32[kept].astype(f)
    Kf, Rf, tf = K32.astype(f), R32.astype(f), t32.astype(f)
    x, y, z = camera(p, Rf, tf)
    a = gf32[:F][kept].astype(f)                                                         # [n, corner q, 3]
    b = gf32[F:2 * F][kept][:, ::-1].astype(f)                                           # the copy's corner 2 - q
    gu, gv, gz = (a[..., j] + b[..., j] for j in range(3))
    s2 = f(2) / f(orig_size)
    iz = f(1) / (z + f(proj_eps))
    gxh = s2 * (gu * Kf[0] - gv * Kf[3])
    gyh = s2 * (gu * Kf[1] - gv * Kf[4])
    gx, gy = gxh * iz, gyh * iz
    gzc = gz - (gxh * x + gyh * y) * iz * iz
    d = np.float64
    terms = [(y * gzc).astype(d) - (z * gy).astype(d), (z * gx).astype(d) - (x * gzc).astype(d), (x * gy).astype(d) - (y * gx).astype(d),
             gx.astype(d), gy.astype(d), gzc.astype(d)]
    g = np.array([float(v.sum()) for v in terms])
    # the absolute-value forms, in float64 (as project_bwd_ref's)
    ap, aK, aR, at = np.abs(p32[kept]).astype(d), np.abs(K32).astype(d), np.abs(R32).astype(d), np.abs(t32).astype(d)
    xa, ya, za = camera(ap, aR, at)
    z64 = np.asarray(z, dtype=d)
    iza = np.abs(np.asarray(iz, dtype=d)) * za / np.abs(z64)
    ua, va, wa = (np.abs(a[..., j]).astype(d) + np.abs(b[..., j]).astype(d) for j in range(3))
    s = 2.0 / float(orig_size)
    gxa, gya = s * (ua * aK[0] + va * aK[3]), s * (ua * aK[1] + va * aK[4])
    gza = wa + (gxa * xa + gya * ya) * iza * iza
    S = np.array([float(v.sum()) for v in (ya * gza + za * gya * iza, za * gxa * iza + xa * gza, xa * gya * iza + ya * gxa * iza,
                                            gxa * iza, gya * iza, gza)])
    return g, S, 3 * int(kept.sum()), kept
