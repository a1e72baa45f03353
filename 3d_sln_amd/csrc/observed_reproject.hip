// An observed depth and label frame of ANY pinhole camera, brought into the refinement view (host/reproject.py; DESIGN §4 "Observed
// frames from any camera").  The frame is a triangle mesh over its pixel grid; sln_raster_forward draws it; the pair ObservedTarget
// takes is read back out of the rasterizer's maps:
//
//   reproject_faces_kernel     a workgroup per tile of 16 x 16 cells of a frame: the 17 x 17 vertices of the tile are unprojected with the
//                              source intrinsics, taken to the target camera by the pose and projected as sln_project_faces projects, ONCE
//                              each, into LDS; every lane then forms the two face slots of its cell (collapsed to (0, 0, 0) without a
//                              reading, across a depth step, nearer than `near`, or in a frame whose focal lengths are not positive), and
//                              the tile's rows leave through LDS as contiguous 8-byte stores (a lane per cell that forms its own four
//                              vertices and stores its own 72 bytes was measured beside it: 15.5 against 10.0 us for one 640 x 480 frame,
//                              137 against 96 us for sixteen - LAB_NOTES §29 - and is not kept);
//   reproject_compose_kernel   per target pixel: the rasterizer's depth (bits untouched) and the label of the source pixel at the hit
//                              face's corner of largest weight, in the row order of the scene tensor's planes; -1 and 0 where nothing was
//                              hit; the hit pixels of a frame counted in a 64-bit integer.
//
// Forward only, no floating-point atomics, no allocation.  Every index that comes out of a map is compared with its range before it
// addresses anything.  Contraction stays on (no -ffp-contract=off for this unit): the test allows four times the fp32 torch restatement's
// own error; the decisions that are part of the definition (reading, depth step) are comparisons of single rounded operations.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "observed_rules.h"
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr float PROJ_EPS = 1e-9f;          // sln_project_faces' eps as host/neural_renderer.py passes it
constexpr int TILE = 16;                   // cells per tile edge; TILE + 1 vertices
constexpr int TV = TILE + 1;
constexpr int CELL_FLOATS = 18;            // two slots of three corners

struct Frame {
  float fx, fy, cx, cy, P[12], K[6], os, near, gap;
  bool ok;
};

__device__ __forceinline__ Frame load_frame(const SlnReproject& d, int b) {
  Frame f;
  const float* k = d.k_src + 4L * b;
  f.fx = k[0]; f.fy = k[1]; f.cx = k[2]; f.cy = k[3];
#pragma unroll
  for (int e = 0; e < 12; ++e) f.P[e] = d.pose[12L * b + e];
#pragma unroll
  for (int e = 0; e < 6; ++e) f.K[e] = d.K_tgt[9L * b + e];
  f.os = d.orig_size; f.near = d.near; f.gap = d.gap;
  f.ok = f.fx > 0.f && f.fy > 0.f;
  return f;
}

// (x_ndc, y_ndc, z_cam, source depth) of the vertex at pixel (i, j); w = 0 marks a pixel without a reading
__device__ __forceinline__ float4 make_vertex(const Frame& f, int i, int j, float dep) {
  const bool reading = obs_reading(dep);
  const float xs = ((float)j + 0.5f - f.cx) / f.fx * dep;
  const float ys = ((float)i + 0.5f - f.cy) / f.fy * dep;
  const float x = xs * f.P[0] + ys * f.P[1] + dep * f.P[2] + f.P[3];
  const float y = xs * f.P[4] + ys * f.P[5] + dep * f.P[6] + f.P[7];
  const float z = xs * f.P[8] + ys * f.P[9] + dep * f.P[10] + f.P[11];
  const float xh = x / (z + PROJ_EPS), yh = y / (z + PROJ_EPS);
  const float u = xh * f.K[0] + yh * f.K[1] + f.K[2];
  const float v = f.os - (xh * f.K[3] + yh * f.K[4] + f.K[5]);
  return make_float4(2.f * (u - f.os / 2.f) / f.os, 2.f * (v - f.os / 2.f) / f.os, z, reading ? dep : 0.f);
}

// one slot: corners p, q, r -> out[9]
__device__ __forceinline__ void make_slot(const Frame& f, const float4& p, const float4& q, const float4& r, float* out) {
  const float dmin = fminf(p.w, fminf(q.w, r.w)), dmax = fmaxf(p.w, fmaxf(q.w, r.w));
  bool cull = !f.ok || !(dmin > 0.f);
  cull = cull || obs_depth_step(dmax, dmin, f.gap);
  cull = cull || !(p.z >= f.near) || !(q.z >= f.near) || !(r.z >= f.near);          // (a NaN depth is culled too)
  out[0] = cull ? 0.f : p.x; out[1] = cull ? 0.f : p.y; out[2] = cull ? 0.f : p.z;
  out[3] = cull ? 0.f : q.x; out[4] = cull ? 0.f : q.y; out[5] = cull ? 0.f : q.z;
  out[6] = cull ? 0.f : r.x; out[7] = cull ? 0.f : r.y; out[8] = cull ? 0.f : r.z;
}

__global__ __launch_bounds__(256) void reproject_faces_kernel(SlnReproject d, float* __restrict__ fxyz) {
  __shared__ float4 vert[TV * TV];
  __shared__ __attribute__((aligned(16))) float stage[TILE * TILE * CELL_FLOATS];
  const int Hc = d.Hs - 1, Wc = d.Ws - 1;
  const int tiles_x = (Wc + TILE - 1) / TILE;
  const int b = blockIdx.y, i0 = (int)(blockIdx.x / tiles_x) * TILE, j0 = (int)(blockIdx.x % tiles_x) * TILE;
  const Frame f = load_frame(d, b);
  const float* dep = d.depth_src + (long)b * d.Hs * d.Ws;
  for (int v = threadIdx.x; v < TV * TV; v += 256) {
    const int i = i0 + v / TV, j = j0 + v % TV;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < d.Hs && j < d.Ws) p = make_vertex(f, i, j, dep[(long)i * d.Ws + j]);
    vert[v] = p;
  }
  __syncthreads();
  const int r = threadIdx.x / TILE, c = threadIdx.x % TILE;
  if (i0 + r < Hc && j0 + c < Wc) {
    const float4 pa = vert[r * TV + c], pb = vert[(r + 1) * TV + c], pc = vert[r * TV + c + 1], pd = vert[(r + 1) * TV + c + 1];
    float* out = stage + (r * TILE + c) * CELL_FLOATS;
    make_slot(f, pa, pb, pc, out);
    make_slot(f, pd, pc, pb, out + 9);
  }
  __syncthreads();
  // a tile row's cells are neighbours in faces_xyz: nc * 18 floats from an even float offset
  const int nc = min(TILE, Wc - j0), nr = min(TILE, Hc - i0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* frame = fxyz + (long)b * Hc * Wc * CELL_FLOATS;
  for (int row = wave; row < nr; row += 4) {
    float2* dst = reinterpret_cast<float2*>(frame + ((long)(i0 + row) * Wc + j0) * CELL_FLOATS);
    const float2* src = reinterpret_cast<const float2*>(stage + row * TILE * CELL_FLOATS);
    for (int e = lane; e < nc * (CELL_FLOATS / 2); e += 64) dst[e] = src[e];
  }
}

__global__ __launch_bounds__(256) void reproject_compose_kernel(const int32_t* __restrict__ fi, const float* __restrict__ weight,
                                                                const float* __restrict__ depth, const unsigned char* __restrict__ labels_src,
                                                                int Hs, int Ws, int S, float* __restrict__ dout,
                                                                unsigned char* __restrict__ lout, unsigned long long* __restrict__ hits) {
  const int b = blockIdx.y;
  const long n = (long)S * S, base = (long)b * n;
  const int F = obs_n_faces(Hs, Ws);
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (p < n) {
    const int y = (int)(p / S), x = (int)(p - (long)y * S);
    const int k = fi[base + p];
    const float* w = weight + 3 * (base + p);
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    hit = obs_hit(k, F, w0, w1, w2);
    unsigned char lab = 0;
    float z = -1.0f;
    if (hit) {
      lab = labels_src[obs_label_index(b, k, w0, w1, w2, Hs, Ws)];
      z = depth[base + p];
    }
    const long q = base + (long)(S - 1 - y) * S + x;             // the planes' rows run downwards
    lout[q] = lab;
    dout[q] = z;
  }
  obs_count_flags(hit, hits + b);
}

}  // namespace

extern "C" {

int sln_reproject_faces(const SlnReproject* d, float* faces_xyz, void* stream) {
  if (!d || !faces_xyz || !d->depth_src || !d->k_src || !d->pose || !d->K_tgt) return SLN_E_BADARG;
  if (obs_check_frames(d->B, d->Hs, d->Ws)) return SLN_E_BADARG;
  if (!(d->orig_size > 0.f) || !(d->gap >= 0.f) || !(d->near > 0.f)) return SLN_E_BADARG;
  if (reinterpret_cast<uintptr_t>(faces_xyz) & 7) return SLN_E_BADARG;
  const int Hc = d->Hs - 1, Wc = d->Ws - 1;
  hipLaunchKernelGGL(reproject_faces_kernel, dim3((unsigned)(sln_cdiv(Wc, TILE) * sln_cdiv(Hc, TILE)), (unsigned)d->B), dim3(256), 0,
                     (hipStream_t)stream, *d, faces_xyz);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_reproject_compose(const int32_t* face_index, const float* weight, const float* raster_depth, const unsigned char* labels_src, int B,
                          int Hs, int Ws, int S, float* depth_out, unsigned char* labels_out, int64_t* hits, void* stream) {
  if (!face_index || !weight || !raster_depth || !labels_src || !depth_out || !labels_out || !hits) return SLN_E_BADARG;
  if (obs_check_frames(B, Hs, Ws) || !obs_target_ok(S)) return SLN_E_BADARG;
  if (reinterpret_cast<uintptr_t>(hits) & 7) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int e = sln_zero_async(hits, sizeof(int64_t) * (size_t)B, st);
  if (e != 0) return e;
  const long n = (long)S * S;
  hipLaunchKernelGGL(reproject_compose_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st, face_index, weight, raster_depth,
                     labels_src, Hs, Ws, S, depth_out, labels_out, reinterpret_cast<unsigned long long*>(hits));
  SLN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
