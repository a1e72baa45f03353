// The pictures the refinement loop saves (testing/test_render_refine.py: save_images :144-163, save_label_depth :118-142, the two label
// statements :343-344), from a scene tensor [B, channels, S, S] that stays on the device (host/scene_pictures.py::scene_pictures_torch
// is the ATen form the tests hold this unit to):
//
//   depth8   d = x - min x;  m = max{d : d < 10};  every d > 10 becomes m;  byte = trunc((d / m) * 255)            (:149-156), float32
//   labels   0 where the float32 sum of the 40 semantic values (channel order) is < 0.5, else 1 + argmax (first maximum)   (:343-344)
//   rgb      palette[labels]                                                                                      (:123-132)
//   masks8   trunc(255 * plane) of the 40 semantic planes                                                         (:159-162)
//
// Three launches on the caller's stream, SP_PX pixels a workgroup, four consecutive pixels a lane in all three:
//   scene_pictures_min / _max   one partial minimum, then one partial maximum of d below 10, per workgroup; every workgroup of the
//                               second re-reduces its room's partial minima.  Min and max do not depend on the order.
//   scene_pictures_pixels       re-reduces both, then walks the 40 semantic planes once with float4 loads, a running argmax and sum in
//                               registers, and stores uchar4.  A room's plane flags (SlnRefineLoss::live_planes) are wave-uniform: a plane
//                               flagged dead enters as 0.f, a plane flagged 1 as 1.f, neither is read.
// status [B]: bit 0 - no d < 10 (non-finite depths; the reference's np.max raises), bit 1 - m == 0 (a constant depth plane; the reference
// divides by zero); the room's depth bytes are 0 in both cases.  A d of exactly 10 is neither replaced nor below the threshold: the
// reference's uint8 cast of (10 / m) * 255 > 255 is undefined, here it saturates at 255 (as does every value above 255; mask values
// outside [0, 1] saturate at 0 / 255 likewise).  No atomics, nothing allocated, nothing read back: legal inside a stream capture and
// bit-identical from call to call.  Contraction is off for this file (build.py): every float32 operation rounds, as numpy's do.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int SP_T = 256;            // threads per workgroup (all three kernels)
constexpr int SP_PX = 4 * SP_T;      // pixels per workgroup
constexpr int SP_SEM = 40;           // semantic planes: channels 1 .. 40
constexpr int SP_CHUNK = 8;          // planes whose loads are in flight together
constexpr float SP_FAR = 10.f;

struct SpWorkspace {                 // per room, G = ceil(S * S / SP_PX) entries each
  float* pmin;
  float* pmax;
};

__host__ __device__ inline int sp_groups(int S) { return (int)(((int64_t)S * S + SP_PX - 1) / SP_PX); }

__host__ __device__ inline SpWorkspace sp_carve(void* ws, int B, int G) {
  SpWorkspace w;
  w.pmin = static_cast<float*>(ws);
  w.pmax = w.pmin + (size_t)B * G;
  return w;
}

__device__ __forceinline__ float sp_block_min(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float sp_block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}

// flag of plane c of room b: 3 (read it) without a table
__device__ __forceinline__ int sp_flag(const unsigned char* __restrict__ live, int b, int channels, int c) {
  return live ? (int)live[(size_t)b * channels + c] : 3;
}

// the four values of a lane's pixels in one plane, as the flag has them
__device__ __forceinline__ float4 sp_load(const float* __restrict__ plane, int64_t p, int flag) {
  if (!(flag & 1)) return make_float4(0.f, 0.f, 0.f, 0.f);
  if (flag == 1) return make_float4(1.f, 1.f, 1.f, 1.f);
  return *reinterpret_cast<const float4*>(plane + p);
}

__device__ __forceinline__ float sp_room_min(const SpWorkspace& ws, int b, int G, float* red) {
  float v = INFINITY;
  for (int g = threadIdx.x; g < G; g += SP_T) v = fminf(v, ws.pmin[(size_t)b * G + g]);
  return sp_block_min(v, red);
}

__global__ void __launch_bounds__(SP_T) scene_pictures_min(const float* __restrict__ image, const unsigned char* __restrict__ live, int channels,
                                                            int64_t n, int G, SpWorkspace ws) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const int64_t p = ((int64_t)blockIdx.x * SP_T + threadIdx.x) * 4;
  float mn = INFINITY;
  if (p < n) {
    const float4 x = sp_load(image + (size_t)b * channels * n, p, sp_flag(live, b, channels, 0));
    mn = fminf(fminf(x.x, x.y), fminf(x.z, x.w));
  }
  mn = sp_block_min(mn, red);
  if (threadIdx.x == 0) ws.pmin[(size_t)b * G + blockIdx.x] = mn;
}

// partial max{d : d < 10}, d = x - min; -inf when the workgroup saw no such value
__global__ void __launch_bounds__(SP_T) scene_pictures_max(const float* __restrict__ image, const unsigned char* __restrict__ live, int channels,
                                                            int64_t n, int G, SpWorkspace ws) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const float mn = sp_room_min(ws, b, G, red);
  const int64_t p = ((int64_t)blockIdx.x * SP_T + threadIdx.x) * 4;
  float mx = -INFINITY;
  if (p < n) {
    const float4 x = sp_load(image + (size_t)b * channels * n, p, sp_flag(live, b, channels, 0));
    const float d[4] = {x.x - mn, x.y - mn, x.z - mn, x.w - mn};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (d[i] < SP_FAR) mx = fmaxf(mx, d[i]);
  }
  mx = sp_block_max(mx, red);
  if (threadIdx.x == 0) ws.pmax[(size_t)b * G + blockIdx.x] = mx;
}

__device__ __forceinline__ unsigned sp_byte(float v) {            // truncation, saturated to a byte (NaN: 0)
  return v >= 255.f ? 255u : (v > 0.f ? (unsigned)(int)v : 0u);
}
__device__ __forceinline__ unsigned sp_pack(unsigned a, unsigned b, unsigned c, unsigned d) { return a | b << 8 | c << 16 | d << 24; }

struct SpParams {
  const float* image;              // [B, channels, S, S]
  const unsigned char* live;       // [B, channels] or NULL
  const uint32_t* palette;         // [41] r | g << 8 | b << 16, or NULL without rgb
  unsigned char* depth8;           // [B, S, S]
  unsigned char* labels;           // [B, S, S] or NULL
  unsigned char* rgb;              // [B, S, S, 3] or NULL
  unsigned char* masks8;           // [B, 40, S, S] or NULL
  int32_t* status;                 // [B]
  SpWorkspace ws;
  int64_t n;                       // S * S
  int channels, G;
};

__global__ void __launch_bounds__(SP_T) scene_pictures_pixels(SpParams q) {
  __shared__ float red[4];
  __shared__ uint32_t pal[SP_SEM + 1];
  const int b = blockIdx.y, channels = q.channels;
  const int64_t n = q.n;
  const float mn = sp_room_min(q.ws, b, q.G, red);
  float m = -INFINITY;
  for (int g = threadIdx.x; g < q.G; g += SP_T) m = fmaxf(m, q.ws.pmax[(size_t)b * q.G + g]);
  m = sp_block_max(m, red);
  const bool none = m == -INFINITY, flat = m == 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) q.status[b] = (none ? 1 : 0) | (flat ? 2 : 0);
  if (q.rgb) {
    if (threadIdx.x <= SP_SEM) pal[threadIdx.x] = q.palette[threadIdx.x];
    __syncthreads();
  }
  const int64_t p = ((int64_t)blockIdx.x * SP_T + threadIdx.x) * 4;
  if (p >= n) return;
  const float* img = q.image + (size_t)b * channels * n;

  {
    const float4 x = sp_load(img, p, sp_flag(q.live, b, channels, 0));
    const float xs[4] = {x.x, x.y, x.z, x.w};
    unsigned by[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float d = xs[i] - mn;
      if (d > SP_FAR) d = m;
      by[i] = (none || flat) ? 0u : sp_byte((d / m) * 255.f);
    }
    *reinterpret_cast<uint32_t*>(q.depth8 + (size_t)b * n + p) = sp_pack(by[0], by[1], by[2], by[3]);
  }
  if (!q.labels && !q.rgb && !q.masks8) return;

  float best[4], sum[4];
  int arg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { best[i] = -INFINITY; sum[i] = 0.f; arg[i] = 0; }
  for (int c0 = 0; c0 < SP_SEM; c0 += SP_CHUNK) {
    float4 v[SP_CHUNK];
#pragma unroll
    for (int j = 0; j < SP_CHUNK; ++j) v[j] = sp_load(img + (size_t)(1 + c0 + j) * n, p, sp_flag(q.live, b, channels, 1 + c0 + j));
#pragma unroll
    for (int j = 0; j < SP_CHUNK; ++j) {
      const float vs[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (vs[i] > best[i]) { best[i] = vs[i]; arg[i] = c0 + j; }
        sum[i] = sum[i] + vs[i];
      }
      if (q.masks8)
        *reinterpret_cast<uint32_t*>(q.masks8 + ((size_t)b * SP_SEM + c0 + j) * n + p) =
            sp_pack(sp_byte(255.f * vs[0]), sp_byte(255.f * vs[1]), sp_byte(255.f * vs[2]), sp_byte(255.f * vs[3]));
    }
  }
  unsigned lab[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) lab[i] = sum[i] < 0.5f ? 0u : (unsigned)(1 + arg[i]);
  if (q.labels) *reinterpret_cast<uint32_t*>(q.labels + (size_t)b * n + p) = sp_pack(lab[0], lab[1], lab[2], lab[3]);
  if (q.rgb) {
    const uint32_t c0 = pal[lab[0]] & 0xffffffu, c1 = pal[lab[1]] & 0xffffffu, c2 = pal[lab[2]] & 0xffffffu, c3 = pal[lab[3]] & 0xffffffu;
    uint32_t* out = reinterpret_cast<uint32_t*>(q.rgb + ((size_t)b * n + p) * 3);       // 12 bytes a lane: r g b r | g b r g | b r g b
    out[0] = c0 | c1 << 24;
    out[1] = c1 >> 8 | c2 << 16;
    out[2] = c2 >> 16 | c3 << 8;
  }
}

}  // namespace

extern "C" int64_t sln_scene_pictures_workspace_bytes(int B, int S) {
  if (B < 1 || S < 1) return SLN_E_BADARG;
  if (S % 4 != 0 || (int64_t)S * S > (int64_t)1 << 30) return SLN_E_UNSUPPORTED;
  return (int64_t)B * sp_groups(S) * 2 * (int64_t)sizeof(float);
}

extern "C" int sln_scene_pictures(const float* image, int B, int channels, int S, const unsigned char* live_planes, const uint32_t* palette,
                                  void* workspace, unsigned char* depth8, unsigned char* labels, unsigned char* rgb, unsigned char* masks8,
                                  int32_t* status, void* stream) {
  if (B < 1 || B > 65535 || S < 1 || S % 4 != 0 || (channels != 41 && channels != 70) || (int64_t)S * S > (int64_t)1 << 30) return SLN_E_UNSUPPORTED;
  if (!image || !workspace || !depth8 || !status || (rgb && !palette)) return SLN_E_BADARG;
  // float4 loads, 32-bit stores of four bytes: the bases must allow them (the plane and room strides do, S % 4 == 0)
  if (reinterpret_cast<uintptr_t>(image) % 16 || reinterpret_cast<uintptr_t>(workspace) % 4 || reinterpret_cast<uintptr_t>(depth8) % 4 ||
      reinterpret_cast<uintptr_t>(labels) % 4 || reinterpret_cast<uintptr_t>(rgb) % 4 || reinterpret_cast<uintptr_t>(masks8) % 4)
    return SLN_E_BADARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int G = sp_groups(S);
  const int64_t n = (int64_t)S * S;
  const SpWorkspace ws = sp_carve(workspace, B, G);
  hipLaunchKernelGGL(scene_pictures_min, dim3(G, B), dim3(SP_T), 0, st, image, live_planes, channels, n, G, ws);
  SLN_CHECK_LAUNCH();
  hipLaunchKernelGGL(scene_pictures_max, dim3(G, B), dim3(SP_T), 0, st, image, live_planes, channels, n, G, ws);
  SLN_CHECK_LAUNCH();
  SpParams q;
  q.image = image; q.live = live_planes; q.palette = palette; q.depth8 = depth8; q.labels = labels; q.rgb = rgb; q.masks8 = masks8;
  q.status = status; q.ws = ws; q.n = n; q.channels = channels; q.G = G;
  hipLaunchKernelGGL(scene_pictures_pixels, dim3(G, B), dim3(SP_T), 0, st, q);
  SLN_CHECK_LAUNCH();
  return 0;
}
