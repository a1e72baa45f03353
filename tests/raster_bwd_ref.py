"""Compositions of the double-sum references of oracle/raster_ref.py that the rasterizer's backward tests share."""
import numpy as np

from oracle import raster_ref as rr


def unflip_hwc(img_chw):
    """[B,3,is,is] as the Renderer returns it (channels first, rows flipped) -> [B,is,is,3] in the rasterizer's row order"""
    return np.ascontiguousarray(np.flip(img_chw, axis=2).transpose(0, 2, 3, 1))


def pixel_map_multi_f64(faces, fi, passes_chw, grads_chw, eps=1e-3):
    """The documented semantics of sln_raster_backward_rgb_multi: the sum over the passes of the dense C = 3 gradient, every
    pass with its own positive-part test.  Returns g64, S, n (added over the passes) and the path counters of the first pass."""
    g = S = n = cnt = None
    for im, gr in zip(passes_chw, grads_chw):
        gi, Si, ni, ci = rr.nmr_backward_pixel_map_f64(faces, fi, unflip_hwc(im), unflip_hwc(gr), eps)
        if g is None:
            g, S, n, cnt = gi, Si, ni, ci
        else:
            g, S, n = g + gi, S + Si, n + ni
    return g, S, n, cnt


def pixel_map_multi_f32(faces, fi, passes_chw, grads_chw, eps=1e-3):
    """the oracle's float path of the same composition: per pass the serial fp32 sum, passes added in fp32"""
    g = np.zeros(faces.shape[:2] + (3, 3), np.float32)
    for im, gr in zip(passes_chw, grads_chw):
        g = g + rr.nmr_backward_pixel_map(faces, fi, unflip_hwc(im), unflip_hwc(gr), eps)
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# fused scene pass at face level
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_backward_f64(faces, face_class, chan, dch, grad_final, acc="f64", pix_eps=1e-3):
    """The algebra of oracle/raster_ref.py::scene_render behind the projection, started from projected faces [B,F,3,3]:
    face_class [B,F] (0 = wall, -1 = none), chan / dch [NC] as sln_scene_forward takes them, grad_final [B,70,is,is].

    The forward maps are nmr_forward's at the two near planes (0.1 for the depth pass, 0.001 for the class passes) and the
    class-pass value is nmr_texture_sample of an all-ones texture; masks, means, wall_max and the 70-channel composition run in
    torch (float64 for acc="f64", float32 for "f32" - scene_render's own path) and autograd gives the depth map's gradient; the two
    raster backwards are the oracle's (_f64 or float) entry points.  acc="f64" returns final, g64, S, n with S and n the sums over
    the depth chain - evaluated at this reference's own depth-map gradient, rounded to fp32 - and the class chain;
    acc="f32" returns final, g32."""
    import torch
    faces = np.ascontiguousarray(faces, np.float32)
    B, F = faces.shape[:2]
    is_ = grad_final.shape[-1]
    NC = len(chan)
    dt = torch.float64 if acc == "f64" else torch.float32
    fiA, wA, dA = rr.nmr_forward(faces, is_, 0.1, 100.0)
    fiB, wB, dB = rr.nmr_forward(faces, is_, 0.001, 100.0)
    val = rr.nmr_texture_sample(faces, np.ones((B, F, 2, 2, 2, 3), np.float32), fiB, wB, dB, 1e-3)        # [B,is,is,3]
    cls_pix = np.where(fiB >= 0, np.take_along_axis(face_class, np.maximum(fiB, 0).reshape(B, -1), 1).reshape(fiB.shape), -1)
    v = val[..., 0]
    img = ((v + v) + v) / np.float32(3.0)                                    # the package's sum of three equal channels / 3, fp32
    raw = torch.from_numpy(np.flip(dA, 1).copy()).to(dt).requires_grad_(True)
    depth = torch.where(raw > 15, torch.full_like(raw, -1.0), raw)
    planes = [[depth[b]] + [torch.zeros(is_, is_, dtype=dt) for _ in range(69)] for b in range(B)]
    for b in range(B):
        wall_max = None
        for c in range(NC):
            image = torch.from_numpy(np.flip(img[b] * (cls_pix[b] == c), 0).copy()).to(dt)
            mask = image > 0.1
            if c == 0:
                wall_max = depth[b][mask].max().detach() if bool(mask.any()) else torch.tensor(10.0, dtype=dt)
            mean = depth[b][mask].mean() if bool(mask.any()) else wall_max
            planes[b][1 + int(chan[c])] = image
            if dch[c] >= 0:
                planes[b][41 + int(dch[c])] = torch.where(mask, depth[b], mean) / wall_max
    final = torch.stack([torch.stack(p) for p in planes])
    (final * torch.from_numpy(np.ascontiguousarray(grad_final)).to(dt)).sum().backward()
    gd = np.ascontiguousarray(np.flip(raw.grad.numpy(), 1)).astype(np.float32)
    passes = []
    for c in range(NC):
        rgb = np.ascontiguousarray(val * (cls_pix == c)[..., None]).astype(np.float32)
        g3 = np.flip(grad_final[:, 1 + int(chan[c])], 1) / np.float32(3.0)
        passes.append((rgb, np.ascontiguousarray(np.repeat(g3[..., None], 3, -1)).astype(np.float32)))
    if acc == "f64":
        g, S, n = rr.nmr_backward_depth_f64(faces, fiA, wA, dA, gd)
        for rgb, g3 in passes:
            gi, Si, ni, _ = rr.nmr_backward_pixel_map_f64(faces, fiB, rgb, g3, pix_eps)
            g, S, n = g + gi, S + Si, n + ni
        return final.detach().numpy(), g, S, n
    g = rr.nmr_backward_depth(faces, fiA, wA, dA, gd)
    for rgb, g3 in passes:
        g = g + rr.nmr_backward_pixel_map(faces, fiB, rgb, g3, pix_eps)
    return final.detach().numpy(), g
