// The 41-channel tensor SPADEGenerator4 consumes, built from the file arrays (colorize_with_spade, testing/test_SPADE_shade.py:50-76;
// host/spade_input.py::build_input is the ATen form, oracle/spade_input_ref.py the numpy one):
//
//   channel 0      ((clip(d - min d, 0, dmax) / dmax) - 0.5) * 2,  dmax = max{d - min d : d - min d < 20}          (:50-55), float32
//   channel 1 + c  the mask of NYU class c: < 120 -> 0, > 120 -> 1, exactly 120 stays 120                          (:56-70)
//   resize         Rh . X . Rw^T in float64 (skimage's internal image), rounded to float32 once                    (:73)
//
// What has to be read is the depth (4 bytes a pixel) and one byte a pixel for every mask that is present; the full-resolution stack
// never exists.  Three launches on the caller's stream:
//   spade_input_min / spade_input_max   SI_G partial minima, then SI_G partial maxima of d - min below 20, per room.  Min and max do
//                                       not depend on the order: the two values are numpy's bit for bit.  They stay on the device.
//   spade_input_resize                  one workgroup per (SI_TR output rows, output channel, room).  It walks the input rows its band
//                                       of Rh covers once, four adjacent columns a lane, transforms each value ON LOAD (normalise /
//                                       threshold / label == 1 + c) and accumulates the SI_TR row sums in float64 registers; the
//                                       [SI_TR, W] float64 result goes to LDS and the band of Rw is applied from there.
// Rh and Rw arrive as banded tables (host/spade_input.py::band_table): per output row the first input index and a fixed-width run of
// float64 weights; an entry of the run that lies outside the resize's support is a true (tiny) matrix entry, never padding.
// A channel without a plane is written as exact 0.0 by its workgroups (the output buffer may hold anything).  No atomics: every sum
// has one fixed order (k ascending), the result is bit-identical from call to call and between a batched and a single call.
// Contraction is off for this file (build.py): the float32 normalisation rounds after every operation like numpy; the float64 sums
// call fma() explicitly.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int SI_G = 128;          // partial results of the depth statistics per room
constexpr int SI_T = 256;          // threads per workgroup (all three kernels)
constexpr int SI_TR = 4;           // output rows per workgroup of the resize
constexpr int SI_C = 41;           // output channels
constexpr int SI_LDS_MAX = 64 * 1024;

struct SiWorkspace {               // per room, SI_G entries each
  float* pmin;
  float* pmax;
  unsigned long long* present;     // label form: bit c set when class c occurs
};

__host__ __device__ inline SiWorkspace si_carve(void* ws, int B) {
  SiWorkspace w;
  w.present = static_cast<unsigned long long*>(ws);
  w.pmin = reinterpret_cast<float*>(w.present + (size_t)B * SI_G);
  w.pmax = w.pmin + (size_t)B * SI_G;
  return w;
}

// LDS column of input column x: one unused float64 behind every 32.  The lanes of the Rw pass read columns `factor` apart (4 at
// 1024 -> 256: 32 bytes, lanes l and l + 8 on the same banks); with the gap lanes 0..31 of a ds_read_b64 touch 32 different bank pairs.
__host__ __device__ __forceinline__ int si_px(int x) { return x + (x >> 5); }

__device__ __forceinline__ float si_block_min(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float si_block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}

// partial minimum of room blockIdx.y's depth; label form: the classes that occur
__global__ void __launch_bounds__(SI_T) spade_input_min(const float* __restrict__ depth, const unsigned char* __restrict__ labels, int64_t n,
                                                         SiWorkspace ws) {
  __shared__ float red[4];
  __shared__ unsigned long long pres[4];
  const int b = blockIdx.y;
  const float* d = depth + (size_t)b * n;
  float mn = INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * SI_T + threadIdx.x; i < n; i += (int64_t)SI_G * SI_T) mn = fminf(mn, d[i]);
  mn = si_block_min(mn, red);
  if (threadIdx.x == 0) ws.pmin[b * SI_G + blockIdx.x] = mn;
  if (labels) {
    const unsigned char* l = labels + (size_t)b * n;
    unsigned long long m = 0;
    for (int64_t i = (int64_t)blockIdx.x * SI_T + threadIdx.x; i < n; i += (int64_t)SI_G * SI_T) {
      const int v = l[i];
      if (v >= 1 && v <= 40) m |= 1ull << (v - 1);
    }
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o, 64);
    if ((threadIdx.x & 63) == 0) pres[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) ws.present[b * SI_G + blockIdx.x] = pres[0] | pres[1] | pres[2] | pres[3];
  }
}

__device__ __forceinline__ float si_room_min(const SiWorkspace& ws, int b, float* red) {
  return si_block_min(threadIdx.x < SI_G ? ws.pmin[b * SI_G + threadIdx.x] : INFINITY, red);
}

// partial max{d - min : d - min < 20}; -inf when the block saw no such value
__global__ void __launch_bounds__(SI_T) spade_input_max(const float* __restrict__ depth, int64_t n, SiWorkspace ws) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const float mn = si_room_min(ws, b, red);
  const float* d = depth + (size_t)b * n;
  float mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * SI_T + threadIdx.x; i < n; i += (int64_t)SI_G * SI_T) {
    const float e = d[i] - mn;
    if (e < 20.f) mx = fmaxf(mx, e);
  }
  mx = si_block_max(mx, red);
  if (threadIdx.x == 0) ws.pmax[b * SI_G + blockIdx.x] = mx;
}

// four adjacent values of one input row; columns at or behind W read as column W - 1 (their sums are never used)
template <typename T>
__device__ __forceinline__ void si_load4(const T* __restrict__ row, int col, int W, bool vec, T v[4]) {
  if (vec) {
    struct alignas(4 * sizeof(T)) V4 { T e[4]; };
    const V4 q = *reinterpret_cast<const V4*>(row + col);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = q.e[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = row[min(col + c, W - 1)];
  }
}

enum { SI_SRC_DEPTH = 0, SI_SRC_U8 = 1, SI_SRC_F32 = 2, SI_SRC_LABEL = 3 };

struct SiParams {
  const float* depth;            // [B, H, W]
  const void* planes;            // masks [B, n_live, H, W] (uint8 / float) or labels [B, H, W] (uint8)
  const int32_t* channels;       // [B, n_live] NYU class of every plane, < 0: padding
  const int32_t* first_h;        // [size]
  const double* w_h;             // [size, width_h]
  const int32_t* first_w;        // [size]
  const double* w_w;             // [width_w, size] (transposed: the lanes of the Rw pass read along `size`)
  float* out;                    // [B, 41, size, size]
  int32_t* status;               // [B]
  SiWorkspace ws;
  int mode, n_live, H, W, size, width_h, width_w, wp;
};

template <int SRC>
__device__ __forceinline__ void si_rows(const SiParams& p, const void* plane, int cls, float mn, float dmax, int lo, int hi, const int* fh,
                                        const double* wl, double* tmp) {
  typedef typename std::conditional<SRC == SI_SRC_DEPTH || SRC == SI_SRC_F32, float, unsigned char>::type T;
  const T* base = static_cast<const T*>(plane);
  const int W = p.W, wh = p.width_h;
  const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(base) % (4 * sizeof(T)) == 0;
  for (int c0 = 4 * threadIdx.x; c0 < W; c0 += 4 * SI_T) {
    double acc[SI_TR][4];
#pragma unroll
    for (int t = 0; t < SI_TR; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][c] = 0.0;
    for (int i0 = lo; i0 < hi; i0 += 4) {
      T raw[4][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) si_load4(base + (size_t)min(i0 + u, p.H - 1) * W, c0, W, vec, raw[u]);     // four rows in flight
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (SRC == SI_SRC_DEPTH) {
            float d = (float)raw[u][c] - mn;
            d = fminf(fmaxf(d, 0.f), dmax) / dmax;             // np.clip(d, 0, dmax) / dmax
            v[c] = (d - 0.5f) * 2.f;
          } else if (SRC == SI_SRC_LABEL) {
            v[c] = (int)raw[u][c] == cls + 1 ? 1.f : 0.f;
          } else {
            const float m = (float)raw[u][c];
            v[c] = m < 120.f ? 0.f : (m > 120.f ? 1.f : m);
          }
        }
#pragma unroll
        for (int t = 0; t < SI_TR; ++t) {
          const int k = i0 + u - fh[t];                        // uniform: a scalar branch
          if ((unsigned)k < (unsigned)wh) {
            const double w = wl[t * wh + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[t][c] = fma(w, (double)v[c], acc[t][c]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < SI_TR; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c0 + c < W) tmp[t * p.wp + si_px(c0 + c)] = acc[t][c];
  }
}

__global__ void __launch_bounds__(SI_T) spade_input_resize(SiParams p) {
  extern __shared__ double lds[];
  __shared__ float red[4];
  __shared__ unsigned long long pres[SI_G];
  const int r0 = blockIdx.x * SI_TR, ch = blockIdx.y, b = blockIdx.z, S = p.size;
  float* out = p.out + ((size_t)(b * SI_C + ch) * S + r0) * S;

  // which plane feeds this channel (uniform for the workgroup)
  int plane = -1;
  float mn = 0.f, dmax = 0.f;
  if (ch == 0) {
    plane = 0;
    mn = si_room_min(p.ws, b, red);
    dmax = si_block_max(threadIdx.x < SI_G ? p.ws.pmax[b * SI_G + threadIdx.x] : -INFINITY, red);
    const bool none = dmax == -INFINITY;                      // np.max of an empty selection: the reference raises
    if (none) dmax = __builtin_nanf("");
    if (blockIdx.x == 0 && threadIdx.x == 0) p.status[b] = none ? 1 : 0;
  } else if (p.mode == SLN_SPADE_INPUT_LABELS) {
    if (threadIdx.x < SI_G) pres[threadIdx.x] = p.ws.present[b * SI_G + threadIdx.x];
    __syncthreads();
    unsigned long long m = 0;
    for (int g = 0; g < SI_G; ++g) m |= pres[g];
    if ((m >> (ch - 1)) & 1ull) plane = 0;
  } else {
    for (int j = p.n_live - 1; j >= 0; --j)
      if (p.channels[b * p.n_live + j] == ch - 1) plane = j;
  }
  if (plane < 0) {
    for (int i = threadIdx.x; i < SI_TR * S; i += SI_T)
      if (r0 + i / S < S) out[i] = 0.f;
    return;
  }

  double* wl = lds;                                   // [SI_TR, width_h]: this tile's rows of the Rh band
  double* tmp = lds + SI_TR * p.width_h;              // [SI_TR, wp]: Rh . X for the tile
  int fh[SI_TR], lo = p.H, hi = 0;
#pragma unroll
  for (int t = 0; t < SI_TR; ++t) {
    const bool live = r0 + t < S;
    fh[t] = live ? min(max(p.first_h[r0 + t], 0), p.H - 1) : p.H;       // a dead row's band starts behind the image
    if (live) { lo = min(lo, fh[t]); hi = max(hi, min(fh[t] + p.width_h, p.H)); }
  }
  for (int i = threadIdx.x; i < SI_TR * p.width_h; i += SI_T) wl[i] = r0 + i / p.width_h < S ? p.w_h[(size_t)r0 * p.width_h + i] : 0.0;
  __syncthreads();

  const size_t hw = (size_t)p.H * p.W;
  if (ch == 0) si_rows<SI_SRC_DEPTH>(p, p.depth + b * hw, 0, mn, dmax, lo, hi, fh, wl, tmp);
  else if (p.mode == SLN_SPADE_INPUT_LABELS) si_rows<SI_SRC_LABEL>(p, static_cast<const unsigned char*>(p.planes) + b * hw, ch - 1, 0.f, 0.f, lo, hi, fh, wl, tmp);
  else if (p.mode == SLN_SPADE_INPUT_MASKS_U8)
    si_rows<SI_SRC_U8>(p, static_cast<const unsigned char*>(p.planes) + ((size_t)b * p.n_live + plane) * hw, 0, 0.f, 0.f, lo, hi, fh, wl, tmp);
  else si_rows<SI_SRC_F32>(p, static_cast<const float*>(p.planes) + ((size_t)b * p.n_live + plane) * hw, 0, 0.f, 0.f, lo, hi, fh, wl, tmp);
  __syncthreads();

  for (int o = threadIdx.x; o < S; o += SI_T) {
    const int fw = min(max(p.first_w[o], 0), p.W - 1);
    double acc[SI_TR];
#pragma unroll
    for (int t = 0; t < SI_TR; ++t) acc[t] = 0.0;
    for (int k = 0; k < p.width_w; ++k) {
      if (fw + k >= p.W) break;
      const double w = p.w_w[(size_t)k * S + o];
      const int x = si_px(fw + k);
#pragma unroll
      for (int t = 0; t < SI_TR; ++t) acc[t] = fma(w, tmp[t * p.wp + x], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < SI_TR; ++t)
      if (r0 + t < S) out[(size_t)t * S + o] = (float)acc[t];
  }
}

size_t si_lds_bytes(int W, int width_h) { return (size_t)SI_TR * ((size_t)si_px(W - 1) + 1 + width_h) * sizeof(double); }

}  // namespace

extern "C" int64_t sln_spade_input_workspace_bytes(int B) {
  if (B < 1) return SLN_E_BADARG;
  return (int64_t)B * SI_G * (sizeof(unsigned long long) + 2 * sizeof(float));
}

extern "C" int sln_spade_input_forward(const float* depth, const void* planes, int mode, const int32_t* channels, int n_live, int B, int H, int W,
                                       int size, const int32_t* first_h, const double* w_h, int width_h, const int32_t* first_w,
                                       const double* w_w, int width_w, void* workspace, float* out, int32_t* status, void* stream) {
  if (!depth || !first_h || !w_h || !first_w || !w_w || !workspace || !out || !status) return SLN_E_BADARG;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || size < 1 || width_h < 1 || width_h > H || width_w < 1 || width_w > W) return SLN_E_BADARG;
  if (mode != SLN_SPADE_INPUT_MASKS_U8 && mode != SLN_SPADE_INPUT_MASKS_F32 && mode != SLN_SPADE_INPUT_LABELS) return SLN_E_BADARG;
  if (mode == SLN_SPADE_INPUT_LABELS) {
    if (!planes) return SLN_E_BADARG;
    n_live = 0;
  } else if (n_live < 0 || n_live > SI_C - 1 || (n_live > 0 && (!planes || !channels))) {
    return SLN_E_BADARG;
  }
  if ((int64_t)H * W > (int64_t)1 << 30 || (int64_t)size * size > (int64_t)1 << 30) return SLN_E_UNSUPPORTED;
  const size_t lds = si_lds_bytes(W, width_h);
  if (lds > (size_t)SI_LDS_MAX) return SLN_E_UNSUPPORTED;          // W up to ~1 900 at the band widths of a 4x reduction
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SiWorkspace ws = si_carve(workspace, B);
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(spade_input_min, dim3(SI_G, B), dim3(SI_T), 0, st, depth,
                     mode == SLN_SPADE_INPUT_LABELS ? static_cast<const unsigned char*>(planes) : nullptr, n, ws);
  SLN_CHECK_LAUNCH();
  hipLaunchKernelGGL(spade_input_max, dim3(SI_G, B), dim3(SI_T), 0, st, depth, n, ws);
  SLN_CHECK_LAUNCH();
  SiParams p;
  p.depth = depth; p.planes = planes; p.channels = channels; p.first_h = first_h; p.w_h = w_h; p.first_w = first_w; p.w_w = w_w;
  p.out = out; p.status = status; p.ws = ws;
  p.mode = mode; p.n_live = n_live; p.H = H; p.W = W; p.size = size; p.width_h = width_h; p.width_w = width_w; p.wp = si_px(W - 1) + 1;
  hipLaunchKernelGGL(spade_input_resize, dim3(sln_cdiv(size, SI_TR), SI_C, B), dim3(SI_T), lds, st, p);
  SLN_CHECK_LAUNCH();
  return 0;
}
