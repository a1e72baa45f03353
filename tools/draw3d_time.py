"""Timing of the 3-D drawing (GPU box): ``ViewRenderer`` alone, then with ``Draw3D`` behind it without and with shadow rays, in ONE process,
per room at 1024 x 1024 / 25 % with 5 candidate views, for 1 room and for 16, and the share of the staged faces the tile cull lets through.

    python tools/draw3d_time.py [repeats]

The bank and the rooms are tools/shade_time.py's: 12 objects per room of a procedural bank (one cuboid model of 1728 faces per class) and
the procedural shell.  Variants are interleaved so that a drift of the machine lands on all of them; per variant the median (p50) and the
spread over `repeats` windows of ITERS calls each (device events around a window), after two warm-up calls of every variant:

  ViewRenderer                 the viewpoint render alone (LAB_NOTES §24's row)
  + Draw3D(shadows=False)      render, then the two launches of sln_draw3d without shadow rays
  + Draw3D(shadows=True)       the same with them
  sln_draw3d alone             the two launches on what the render left, without and with shadow rays

The cull's share is counted in torch by the kernel's own rule (csrc/draw3d.hip: per tile the padded box of the offset hit points of the
samples that cast a ray and the lamp, against the box of every chunk of 256 faces and then against every face's box of the chunks that
pass): chunks staged / chunks offered and faces kept / faces staged, over the tiles that cast a ray at all.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SH = importlib.import_module("3d_sln_amd.host.shade")
RF = importlib.import_module("3d_sln_amd.host.refine")
D = importlib.import_module("3d_sln_amd.host.draw3d")
import shade_time as ST      # noqa: E402

ITERS = int(os.environ.get("ITERS", "10"))
SIZE, VIEWS, PERCENT = int(os.environ.get("SIZE", "1024")), 5, 25
CHUNK = 256                  # faces per chunk of csrc/draw3d.hip


def rooms(bank, R):
    parts = [ST.room(bank, seed=s) for s in range(R)]
    return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), [p[3][0] for p in parts])


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / ITERS * 1e-3


def cull_share(r, draw):
    """(faces kept, chunks staged, chunks offered, tiles that cast a ray, tiles) by the kernel's rule, room by room on the device"""
    k, S, F = draw.k, r.size, r.F
    T = k * (16 // k)
    nt = (S + T - 1) // T
    kept = boxed = chunks = offered = casting = 0
    for room in range(r.batch):
        b = room * r.views + int(r.chosen[room])
        pts, (ax, bx, ay, by) = D.camera_faces(r.faces_xyz[b], draw.K[b], S)
        v0, e1, e2 = pts[:, 0], pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0]
        flat = ((e1 == 0) & (e2 == 0)).all(-1)
        lo = torch.where(flat[:, None], torch.full_like(v0, 3e38), pts.amin(1))
        hi = torch.where(flat[:, None], torch.full_like(v0, -3e38), pts.amax(1))
        fi = r.face_index[b].long()
        hit = (fi >= 0) & (fi < F)
        fc = fi.clamp(0, F - 1)
        z = r._raster_depth[b]
        pc = (2 * torch.arange(S, device=z.device) + 1 - S).float() / S
        p = torch.stack(((pc[None, :] * ax + bx) * z, (pc[:, None] * ay + by) * z, z), -1)
        n = D._cross(e1[fc], e2[fc])
        n = n / torch.sqrt(D._dot(n, n).clamp(min=1e-30))[..., None]
        n = torch.where((D._dot(n, p) > 0)[..., None], -n, n)
        light = draw.light_cam[room]
        l = light - p
        need = hit & (D._dot(n, l) > 0)
        o = p + D.BIAS * n
        pad_to = nt * T - S
        big = torch.full_like(o, 3e38)
        olo = torch.nn.functional.pad(torch.where(need[..., None], o, big), (0, 0, 0, pad_to, 0, pad_to), value=3e38)
        ohi = torch.nn.functional.pad(torch.where(need[..., None], o, -big), (0, 0, 0, pad_to, 0, pad_to), value=-3e38)
        tlo = olo.reshape(nt, T, nt, T, 3).amin(dim=(1, 3)).reshape(-1, 3)
        thi = ohi.reshape(nt, T, nt, T, 3).amax(dim=(1, 3)).reshape(-1, 3)
        cast = tlo[:, 0] <= thi[:, 0]
        # the cone from the lamp: axis to the middle of the tile's offset hit points, half angle the largest of its segments'
        axis = torch.where(cast[:, None], 0.5 * (tlo + thi) - light, torch.ones_like(tlo))
        axis = axis / torch.sqrt(D._dot(axis, axis).clamp(min=1e-30))[:, None]
        w = torch.nn.functional.pad(o - light, (0, 0, 0, pad_to, 0, pad_to)).reshape(nt, T, nt, T, 3)
        w = w / torch.sqrt(D._dot(w, w).clamp(min=1e-30))[..., None]
        live = torch.nn.functional.pad(need, (0, pad_to, 0, pad_to)).reshape(nt, T, nt, T)
        ab = axis.reshape(nt, 1, nt, 1, 3)
        sin_t = torch.where(live, torch.sqrt(D._dot(D._cross(w, ab.expand_as(w)), D._cross(w, ab.expand_as(w)))), torch.zeros_like(w[..., 0])).amax(dim=(1, 3)).reshape(-1)
        cos_min = torch.where(live, D._dot(w, ab), torch.ones_like(w[..., 0])).amin(dim=(1, 3)).reshape(-1)
        sin_t = (sin_t + 1e-4).clamp(max=1.0)
        cos_t = torch.sqrt((1.0 - sin_t * sin_t).clamp(min=0.0))
        axis, sin_t, cos_t, cone = axis[cast], sin_t[cast], cos_t[cast], (cos_min > 0.1)[cast]
        tlo, thi = torch.minimum(tlo, light)[cast], torch.maximum(thi, light)[cast]
        pad = 1e-3 * torch.maximum(tlo.abs(), thi.abs()).amax(1).clamp(min=1.0)
        half = 0.5 * (hi - lo)
        mid_v, rho0 = lo + half - light, torch.sqrt(D._dot(half, half))
        fill = (-F) % CHUNK
        clo = torch.cat((lo, torch.full((fill, 3), 3e38, device=lo.device))).reshape(-1, CHUNK, 3).amin(1)
        chi = torch.cat((hi, torch.full((fill, 3), -3e38, device=hi.device))).reshape(-1, CHUNK, 3).amax(1)
        for a in range(0, tlo.shape[0], 512):
            s = slice(a, a + 512)
            top, bottom = (thi[s] + pad[s, None])[:, None], (tlo[s] - pad[s, None])[:, None]
            in_box = ((lo[None] <= top) & (hi[None] >= bottom)).all(-1)
            along = D._dot(mid_v[None], axis[s, None])
            off = torch.sqrt(D._dot(D._cross(mid_v[None].expand(along.shape[0], -1, -1), axis[s, None].expand(-1, F, -1)),
                                    D._cross(mid_v[None].expand(along.shape[0], -1, -1), axis[s, None].expand(-1, F, -1))))
            in_cone = ~cone[s, None] | (off * cos_t[s, None] - along * sin_t[s, None] <= rho0[None] + pad[s, None])
            boxed += int(in_box.sum())
            kept += int((in_box & in_cone).sum())
            chunks += int(((clo[None] <= top) & (chi[None] >= bottom)).all(-1).sum())
        offered += int(cast.sum()) * clo.shape[0]
        casting += int(cast.sum())
    return kept, boxed, chunks, offered, casting, r.batch * nt * nt


def measure(bank, R, repeats):
    boxes, angles, objs, rows = rooms(bank, R)
    draws = torch.rand(R, VIEWS, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    r = SH.ViewRenderer(bank, size=SIZE, views=VIEWS, batch=R)
    plain, lit = D.Draw3D(r, percentage=PERCENT, shadows=False), D.Draw3D(r, percentage=PERCENT, shadows=True)
    args = (boxes, angles, objs, rows)
    variants = [("ViewRenderer", lambda: r(*args, draws=draws)), ("+ Draw3D(shadows=False)", lambda: plain.draw3d(*args, draws=draws)),
                ("+ Draw3D(shadows=True)", lambda: lit.draw3d(*args, draws=draws)), ("sln_draw3d alone, no shadows", plain.draw3d),
                ("sln_draw3d alone, shadows", lit.draw3d)]
    for _, fn in variants[:3] + variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    print("%d room(s) x %d views at %d x %d, picture %d x %d (k = %d), %d face slots per room; %d windows of %d calls; per ROOM: p50 [min .. max]"
          % (R, VIEWS, SIZE, SIZE, lit.P, lit.P, lit.k, r.F, repeats, ITERS), flush=True)
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window(fn) / R)
    for name, _ in variants:
        v = sorted(times[name])
        print("   %-30s %10.1f us  [%9.1f .. %9.1f]" % (name, v[len(v) // 2] * 1e6, v[0] * 1e6, v[-1] * 1e6), flush=True)
    kept, boxed, chunks, offered, casting, tiles = cull_share(r, lit)
    print("   tile cull over the %d of %d tiles that cast a ray: %d of %d chunks of %d faces staged (%.2f %%), %d of their %d faces kept (%.2f %%; "
          "%.3f %% of all; the box test alone would keep %d, %.2f %% of all); accepted views %s, status %s"
          % (casting, tiles, chunks, offered, CHUNK, 100.0 * chunks / max(offered, 1), kept, chunks * CHUNK, 100.0 * kept / max(chunks * CHUNK, 1),
             100.0 * kept / max(offered * CHUNK, 1), boxed, 100.0 * boxed / max(offered * CHUNK, 1), r.chosen.tolist(), r.status.tolist()), flush=True)
    dark = float((lit.picture.float().sum(-1) < plain.picture.float().sum(-1)).float().mean())
    print("   [check] %.1f %% of the output pixels are darker with shadows, none brighter: %s"
          % (100 * dark, bool((lit.picture.int() <= plain.picture.int() + 1).all())), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("draw3d_time.py measures on the GPU; none found")
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    names = [n for n in importlib.import_module("3d_sln_amd.host.synthetic").FURNITURE if n in SH.NYU40]
    bank = RF.MeshBank(names, "cuda", subdiv=12)
    for R in (1, 16):
        measure(bank, R, repeats)


if __name__ == "__main__":
    main()
