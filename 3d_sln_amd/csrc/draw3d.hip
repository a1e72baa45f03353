// The --draw_3d picture of a layout (render/render_room_color.py::render_test behind render_caller.py), from what the viewpoint render
// (shade_view.hip + sln_raster_forward) leaves on the device: a lit colour picture of the accepted view with hard shadows.  The shading
// model is this project's, not Blender's ("3-D drawing"); everything is in the chosen view's camera frame.
//
//   draw3d_faces_kernel   R x F lanes: the chosen view's faces back from (x_ndc, y_ndc, z_cam) to camera space; per face v0, e1, e2 and
//                         its bounding box, 16 floats, into the workspace, and per workgroup - a chunk of 256 face slots - the box of the
//                         chunk.  `chosen` is read here, on the device.
//   draw3d_light_kernel   256 lanes own a T x T tile of raster samples (T = k * (16 / k): a whole number of output pixels).  A lane forms
//                         its hit point, the two-sided normal and the light term; lanes that need a shadow ray reduce the box of their
//                         offset hit points, which together with the lamp bounds every segment of the tile.  The faces are walked in
//                         chunks of 256: a chunk whose box misses that bound is skipped (the same decision in every lane; without it the
//                         4 096 tiles of a 1024^2 picture read every face's box: LAB_NOTES §27); otherwise each lane tests ONE
//                         face's box, the survivors are compacted (ballot order) into an LDS list, and every lane walks the list - all
//                         lanes read the same LDS record, a broadcast - with a two-sided Moller-Trumbore test.  The tile's linear colours
//                         go to LDS, lanes 0 .. (T / k)^2 - 1 add their k x k samples row by row, encode sRGB and store three bytes.
//
// The cull only drops faces whose box misses the (padded) box of the segments' end points, which contains every segment: results do not
// depend on it.  No atomics, no allocation, fixed-order sums: the same bytes from call to call.  Every index read from device memory
// (face_index, face_label, chosen) is clamped or compared with its range before it is used.  Contraction stays on, as in shade_view.hip.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int CHUNK = 256;               // faces staged per pass: one per lane of the cull
constexpr int REC = 16;                  // floats per face in the workspace
constexpr float BIG = 3.0e38f;
constexpr float TINY = 1e-30f;

struct View { float ax, bx, ay, by; };   // x / z = x_ndc * ax + bx,  y / z = y_ndc * ay + by

__device__ __forceinline__ View view_of(const float* __restrict__ K, float S) {
  const float fx = K[0], cx = K[2], fy = K[4], cy = K[5];
  View v;
  v.ax = S / (2.f * fx); v.bx = (S / 2.f - cx) / fx;
  v.ay = -S / (2.f * fy); v.by = (S / 2.f - cy) / fy;
  return v;
}

__device__ __forceinline__ int chosen_view(const int64_t* __restrict__ chosen, int r, int V) {
  const int64_t c = chosen[r];
  return c < 0 ? 0 : (c >= V ? V - 1 : (int)c);
}

__device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// 256 lanes: lo / hi [3] of every lane -> the box of the whole workgroup in every lane (s_box: 24 floats)
__device__ __forceinline__ void block_box(float lo[3], float hi[3], float* s_box) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 3; ++e) { lo[e] = wave_min(lo[e]); hi[e] = wave_max(hi[e]); }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int e = 0; e < 3; ++e) { s_box[6 * wave + e] = lo[e]; s_box[6 * wave + 3 + e] = hi[e]; }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    lo[e] = fminf(fminf(s_box[e], s_box[6 + e]), fminf(s_box[12 + e], s_box[18 + e]));
    hi[e] = fmaxf(fmaxf(s_box[3 + e], s_box[9 + e]), fmaxf(s_box[15 + e], s_box[21 + e]));
  }
}

// one workgroup per chunk of CHUNK face slots: the slots' records, and the box of the chunk behind them
__global__ __launch_bounds__(256) void draw3d_faces_kernel(SlnDraw3D d, float4* __restrict__ ws, float4* __restrict__ chunk_box) {
  __shared__ float s_box[4 * 6];
  const int f = blockIdx.x * CHUNK + threadIdx.x, r = blockIdx.y;
  const bool in = f < d.F;
  const long b = (long)r * d.V + chosen_view(d.chosen, r, d.V);
  const View vw = view_of(d.K + 9 * b, (float)d.S);
  const float* c = d.faces_xyz + 9L * (b * d.F + (in ? f : d.F - 1));
  float p[3][3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float z = c[3 * q + 2];
    p[q][0] = (c[3 * q] * vw.ax + vw.bx) * z;
    p[q][1] = (c[3 * q + 1] * vw.ay + vw.by) * z;
    p[q][2] = z;
  }
  float e1[3], e2[3], lo[3], hi[3];
  bool flat = true;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    e1[e] = p[1][e] - p[0][e];
    e2[e] = p[2][e] - p[0][e];
    flat = flat && e1[e] == 0.f && e2[e] == 0.f;
    lo[e] = fminf(p[0][e], fminf(p[1][e], p[2][e]));
    hi[e] = fmaxf(p[0][e], fmaxf(p[1][e], p[2][e]));
  }
  if (flat || !in) {                      // a collapsed slot has a zero determinant for every ray: an empty box, the cull drops it
#pragma unroll
    for (int e = 0; e < 3; ++e) { lo[e] = BIG; hi[e] = -BIG; }
  }
  if (in) {
    float4* out = ws + 4L * ((long)r * d.F + f);
    out[0] = make_float4(p[0][0], p[0][1], p[0][2], e1[0]);
    out[1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    out[2] = make_float4(e2[2], lo[0], lo[1], lo[2]);
    out[3] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
  block_box(lo, hi, s_box);               // (a chunk of empty slots keeps an empty box: it is never staged)
  if (threadIdx.x == 0) {
    float4* out = chunk_box + 2L * ((long)r * gridDim.x + blockIdx.x);
    out[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    out[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
}

__device__ __forceinline__ float srgb_encode(float c) {
  c = fminf(fmaxf(c, 0.f), 1.f);
  return c <= 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.f / 2.4f) - 0.055f;
}

__global__ __launch_bounds__(256) void draw3d_light_kernel(SlnDraw3D d, const float4* __restrict__ ws, const float4* __restrict__ chunk_box, int T,
                                                           unsigned char* __restrict__ picture, float* __restrict__ linear) {
  __shared__ float4 s_face[CHUNK * 3];     // v0 e1 e2 and the face's index (as bits) of the chunk's survivors
  __shared__ float s_lin[256 * 3];
  __shared__ float s_box[4 * 6];
  __shared__ int s_cnt[4];
  __shared__ float s_red[8];
  const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
  const int r = blockIdx.z, S = d.S, F = d.F, k = d.k;
  const long b = (long)r * d.V + chosen_view(d.chosen, r, d.V);
  const View vw = view_of(d.K + 9 * b, (float)S);
  const float4* room = ws + 4L * (long)r * F;

  const int ty = lane / T, tx = lane - ty * T;
  const int yi = blockIdx.y * T + ty, xi = blockIdx.x * T + tx;
  const bool valid = ty < T && yi < S && xi < S;
  const long at = b * S * S + (long)(valid ? yi : 0) * S + (valid ? xi : 0);
  const int fi = d.face_index[at];
  const float z = d.depth[at];
  const bool hit = valid && fi >= 0 && fi < F;
  const int fc = hit ? fi : 0;
  const float4 q0 = room[4L * fc], q1 = room[4L * fc + 1], q2 = room[4L * fc + 2];
  const unsigned char lab = d.face_label[(long)r * F + fc];
  const int li = lab <= 40 ? lab : 0;
  const float alb[3] = {d.albedo[3 * li], d.albedo[3 * li + 1], d.albedo[3 * li + 2]};
  const float lx = d.light_cam[3 * r], ly = d.light_cam[3 * r + 1], lz = d.light_cam[3 * r + 2];

  // the hit point, the two-sided normal, the light term
  const float xp = (float)(2 * xi + 1 - S) / (float)S, yp = (float)(2 * yi + 1 - S) / (float)S;
  const float px = (xp * vw.ax + vw.bx) * z, py = (yp * vw.ay + vw.by) * z, pz = z;
  const float e1x = q0.w, e1y = q1.x, e1z = q1.y, e2x = q1.z, e2y = q1.w, e2z = q2.x;
  float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float inv_n = 1.f / sqrtf(fmaxf(nx * nx + ny * ny + nz * nz, TINY));
  const float sgn = (nx * px + ny * py + nz * pz) > 0.f ? -inv_n : inv_n;
  nx *= sgn; ny *= sgn; nz *= sgn;
  const float tlx = lx - px, tly = ly - py, tlz = lz - pz;
  const float ll = tlx * tlx + tly * tly + tlz * tlz;
  const float d2 = fmaxf(ll, d.min_dist * d.min_dist);
  const float c = fmaxf(0.f, (nx * tlx + ny * tly + nz * tlz) / sqrtf(fmaxf(ll, TINY)));
  const bool need = hit && d.shadows != 0 && c > 0.f;
  const float ox = px + d.bias * nx, oy = py + d.bias * ny, oz = pz + d.bias * nz;
  const float dx = lx - ox, dy = ly - oy, dz = lz - oz;

  // the box of the tile's segments: the offset hit points of the lanes that cast a ray, and the lamp
  float lo[3] = {need ? ox : BIG, need ? oy : BIG, need ? oz : BIG}, hi[3] = {need ? ox : -BIG, need ? oy : -BIG, need ? oz : -BIG};
  block_box(lo, hi, s_box);
  const bool any = lo[0] <= hi[0];                                   // uniform over the workgroup
  bool shadowed = false;
  if (any) {
    const float lc[3] = {lx, ly, lz};
    const float mid[3] = {lo[0] + hi[0], lo[1] + hi[1], lo[2] + hi[2]};       // twice the middle of the offset hit points' box
    float reach = 1.f;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      lo[e] = fminf(lo[e], lc[e]); hi[e] = fmaxf(hi[e], lc[e]);
      reach = fmaxf(reach, fmaxf(fabsf(lo[e]), fabsf(hi[e])));
    }
    const float pad = 1e-3f * reach;                                 // far above what fp32 rounding moves a corner or a hit point by
    // every segment ends at the lamp: they also lie in the cone from the lamp around the axis to the middle of the hit points' box whose
    // half angle is the largest of the segments' (widened by 1e-4 rad).  A face is kept only if the sphere around its box reaches into
    // that cone; a bundle wider than about 84 degrees is bounded by the box alone.
    float ax = 0.5f * mid[0] - lx, ay = 0.5f * mid[1] - ly, az = 0.5f * mid[2] - lz;
    const float an = 1.f / sqrtf(fmaxf(ax * ax + ay * ay + az * az, TINY));
    ax *= an; ay *= an; az *= an;
    const float wx = -dx, wy = -dy, wz = -dz;                        // lamp -> the lane's offset hit point
    const float wn = 1.f / sqrtf(fmaxf(wx * wx + wy * wy + wz * wz, TINY));
    const float cx_ = wy * az - wz * ay, cy_ = wz * ax - wx * az, cz_ = wx * ay - wy * ax;
    const float sin_i = need ? sqrtf(cx_ * cx_ + cy_ * cy_ + cz_ * cz_) * wn : 0.f;
    const float cos_i = need ? (wx * ax + wy * ay + wz * az) * wn : 1.f;
    float s_max = wave_max(sin_i), c_min = wave_min(cos_i);
    if (wl == 0) { s_red[wave] = s_max; s_red[4 + wave] = c_min; }
    __syncthreads();
    s_max = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    c_min = fminf(fminf(s_red[4], s_red[5]), fminf(s_red[6], s_red[7]));
    const bool cone = c_min > 0.1f;
    const float sin_t = fminf(s_max + 1e-4f, 1.f), cos_t = sqrtf(fmaxf(1.f - sin_t * sin_t, 0.f));
#pragma unroll
    for (int e = 0; e < 3; ++e) { lo[e] -= pad; hi[e] += pad; }
    const float4* cbox = chunk_box + 2L * (long)r * ((F + CHUNK - 1) / CHUNK);
    for (int c0 = 0; c0 < F; c0 += CHUNK) {
      // the chunk's own box first: the same for every lane, a chunk that misses the bundle is not staged at all
      const float4 cl = cbox[2 * (c0 / CHUNK)], ch = cbox[2 * (c0 / CHUNK) + 1];
      if (!(cl.x <= hi[0] && ch.x >= lo[0] && cl.y <= hi[1] && ch.y >= lo[1] && cl.z <= hi[2] && ch.z >= lo[2])) continue;
      const int g = c0 + lane;
      const int gc = g < F ? g : F - 1;
      const float4 g0 = room[4L * gc], g1 = room[4L * gc + 1], g2 = room[4L * gc + 2], g3 = room[4L * gc + 3];
      const bool in_box = g < F && g2.y <= hi[0] && g3.x >= lo[0] && g2.z <= hi[1] && g3.y >= lo[1] && g2.w <= hi[2] && g3.z >= lo[2];
      const float hx = 0.5f * (g3.x - g2.y), hy = 0.5f * (g3.y - g2.z), hz = 0.5f * (g3.z - g2.w);
      const float rho = sqrtf(hx * hx + hy * hy + hz * hz) + pad;
      const float vx = g2.y + hx - lx, vy = g2.z + hy - ly, vz = g2.w + hz - lz;       // lamp -> the middle of the face's box
      const float along = vx * ax + vy * ay + vz * az;
      const float ux = vy * az - vz * ay, uy = vz * ax - vx * az, uz = vx * ay - vy * ax;   // (|v x a|: no cancellation near the axis)
      const float off = sqrtf(ux * ux + uy * uy + uz * uz);
      const bool keep = in_box && (!cone || off * cos_t - along * sin_t <= rho);
      const unsigned long long m = __ballot(keep);
      if (wl == 0) s_cnt[wave] = __popcll(m);
      __syncthreads();
      int slot = __popcll(m & ((1ull << wl) - 1ull)), total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int n = s_cnt[w];
        slot += w < wave ? n : 0;
        total += n;
      }
      if (keep) {
        s_face[3 * slot] = g0;
        s_face[3 * slot + 1] = g1;
        s_face[3 * slot + 2] = make_float4(g2.x, __int_as_float(g), 0.f, 0.f);
      }
      __syncthreads();
      for (int j = 0; j < total; ++j) {
        const float4 a0 = s_face[3 * j], a1 = s_face[3 * j + 1], a2 = s_face[3 * j + 2];
        // v0 = a0.xyz, e1 = (a0.w, a1.x, a1.y), e2 = (a1.z, a1.w, a2.x)
        const float pvx = dy * a2.x - dz * a1.w, pvy = dz * a1.z - dx * a2.x, pvz = dx * a1.w - dy * a1.z;
        const float det = a0.w * pvx + a1.x * pvy + a1.y * pvz;
        const float inv = 1.f / det;
        const float tvx = ox - a0.x, tvy = oy - a0.y, tvz = oz - a0.z;
        const float u = (tvx * pvx + tvy * pvy + tvz * pvz) * inv;
        const float qx = tvy * a1.y - tvz * a1.x, qy = tvz * a0.w - tvx * a1.y, qz = tvx * a1.x - tvy * a0.w;
        const float v = (dx * qx + dy * qy + dz * qz) * inv;
        const float t = (a1.z * qx + a1.w * qy + a2.x * qz) * inv;
        const bool h = det != 0.f && u >= 0.f && v >= 0.f && u + v <= 1.f && t > 0.f && t < 1.f && __float_as_int(a2.y) != fi;
        shadowed = shadowed || (need && h);
      }
      __syncthreads();
    }
  }

  const float E = d.ambient + (shadowed ? 0.f : d.intensity * c / d2);
  float col[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) col[e] = hit ? alb[e] * E : d.background[e];
  if (valid && linear) {
    float* o = linear + 3L * (((long)r * S + yi) * S + xi);
    o[0] = col[0]; o[1] = col[1]; o[2] = col[2];
  }
  s_lin[3 * lane] = col[0]; s_lin[3 * lane + 1] = col[1]; s_lin[3 * lane + 2] = col[2];
  __syncthreads();

  // the box filter: lanes 0 .. (T / k)^2 - 1, k x k samples row by row, then the sRGB bytes in image row order
  const int np = T / k, P = S / k;
  const int oy_t = lane / np, ox_t = lane - oy_t * np;
  const int Y = blockIdx.y * np + oy_t, X = blockIdx.x * np + ox_t;
  if (oy_t < np && Y < P && X < P) {
    float sum[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < k; ++i) {
        const int s = (oy_t * k + j) * T + ox_t * k + i;
        sum[0] += s_lin[3 * s]; sum[1] += s_lin[3 * s + 1]; sum[2] += s_lin[3 * s + 2];
      }
    const float n = (float)(k * k);
    unsigned char* o = picture + 3L * (((long)r * P + (P - 1 - Y)) * P + X);
#pragma unroll
    for (int e = 0; e < 3; ++e) o[e] = (unsigned char)floorf(srgb_encode(sum[e] / n) * 255.f + 0.5f);
  }
}

}  // namespace

extern "C" {

int64_t sln_draw3d_workspace_bytes(int R, int F) {
  if (R < 1 || R > 65535 || F < 1 || F > (1 << 24)) return SLN_E_BADARG;
  return ((int64_t)R * F * REC + (int64_t)R * ((F + CHUNK - 1) / CHUNK) * 8) * (int64_t)sizeof(float);
}

int sln_draw3d(const SlnDraw3D* d, void* workspace, unsigned char* picture, float* linear, void* stream) {
  if (!d || !workspace || !picture) return SLN_E_BADARG;
  if (!d->faces_xyz || !d->face_index || !d->depth || !d->face_label || !d->chosen || !d->K || !d->light_cam || !d->albedo) return SLN_E_BADARG;
  if (d->R < 1 || d->V < 1 || d->F < 1 || d->S < 1 || d->k < 1) return SLN_E_BADARG;
  if (d->k > 16 || d->S % d->k != 0 || d->S > 32768 || (long)d->R * d->V > 65535 || d->F > (1 << 24)) return SLN_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  float4* faces = static_cast<float4*>(workspace);
  float4* chunk_box = faces + 4L * d->R * d->F;                       // [R, ceil(F / CHUNK), 2] behind the face records
  hipLaunchKernelGGL(draw3d_faces_kernel, dim3((unsigned)((d->F + CHUNK - 1) / CHUNK), (unsigned)d->R), dim3(256), 0, st, *d, faces, chunk_box);
  const int T = d->k * (16 / d->k);
  const unsigned tiles = (unsigned)((d->S + T - 1) / T);
  hipLaunchKernelGGL(draw3d_light_kernel, dim3(tiles, tiles, (unsigned)d->R), dim3(256), 0, st, *d, static_cast<const float4*>(faces),
                     static_cast<const float4*>(chunk_box), T, picture, linear);
  SLN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
