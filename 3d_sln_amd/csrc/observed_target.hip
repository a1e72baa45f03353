// The refinement target of an OBSERVED room: from a metric depth image and a class-index image (uint8, 0 = no class, 1 + c = NYU class c:
// what host/scene_pictures.py and spade_input.InputBuilder(labels=) exchange) to the 70-plane tensor the refinement loss consumes - the
// tensor sln_scene_forward composes from its own rasterisation (raster.hip: the statistics of the class pass, compose_tables,
// scene_compose_kernel), composed here from images nobody rasterised.  host/observe.py::observed_target_torch is the ATen form the tests
// hold this unit to.  Per room, with d the depth and y the label byte of a pixel:
//
//   reading     0 < d <= 15 (a NaN, an infinity, d <= 0 and d > 15 are no readings);  d0 = d with a reading, else -1 (depth_value's background)
//   l           y where y <= 40 and the pixel has a reading, else 0
//   plane 0     d0
//   plane 1+c   1.0 where l == 1 + c, else 0.0                                                          c = 0 .. 39
//   statistics  per label value v = 1 .. 40 over {l == v}: the pixel count, the sum of rint((double)d0 * 2^32) in a 64-bit integer (order
//               independent; converted to double once, times 2^-32 - the scene pass's fixed point) and the maximum of d0
//   wall_max    the maximum over {l == chan[0] + 1}, 10 where that mask is empty
//   plane 41+k  for the class c with dch[c] == k:  d0 / wall_max inside {l == chan[c] + 1},  fill_c / wall_max outside,
//               fill_c = cnt_c > 0 ? (float)(sum_c / cnt_c) : wall_max;  all 0 for a k no class owns
//   status      bit 0: a label byte > 40;  bit 1: an l > 0 whose NYU channel no class has;  bit 2: no wall pixel;
//               bit 3: a byte in 1 .. 40 on a pixel without a reading
//
// Two launches on the caller's stream, four consecutive pixels a lane in both:
//   observed_stats     a workgroup per (room, label value) strides the label image (one 4-byte load per four pixels; the 16-byte depth
//                      load only where one of the four bytes is the workgroup's) and reduces count, integer sum and maximum in a fixed LDS
//                      tree; workgroup 40 of a room strides both images for the status bits.  Every statistic is an integer sum, a maximum
//                      or an OR: the bits do not depend on any order.
//   observed_compose   the derived tables (owner label, fill / wall_max per depth channel, wall_max) go to LDS once per workgroup; a lane
//                      then issues one 16-byte store per plane, a wavefront 1 KiB of one plane per store instruction.
// The class tables are HOST arrays: they are checked before anything is launched and travel as launch arguments (132 bytes).  No
// allocation, no synchronisation, nothing read back, no floating-point atomics: legal inside a stream capture and bit-identical from
// call to call.  Contraction is off for this file (build.py); every quotient is a correctly rounded float32 division, as the scene pass's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "observed_rules.h"
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int OT_T = 256;            // threads per workgroup (both kernels)
constexpr int OT_LAB = 40;           // label values 1 .. 40
constexpr int OT_SEM0 = 1;           // first semantic plane
constexpr int OT_DEP0 = 41;          // first depth-hot plane
constexpr int OT_MAX_DCH = 31;       // nch <= 72

struct OtRoom {                      // the statistics of one room (4-byte aligned: the 64-bit sums are kept as two halves)
  uint32_t sum_lo[OT_LAB], sum_hi[OT_LAB];
  int32_t cnt[OT_LAB];
  float mx[OT_LAB];
  int32_t flags, pad_;
};

struct OtTabs {                      // derived from chan / dch on the host
  int32_t own_label[OT_MAX_DCH + 1]; // label value (chan + 1) of the class owning depth channel k, 0: nobody
  int32_t wall_label;                // chan[0] + 1
};

__global__ void __launch_bounds__(OT_T) observed_stats(const float* __restrict__ depth, const unsigned char* __restrict__ labels, int64_t n,
                                                      unsigned long long known, OtRoom* __restrict__ ws) {
  __shared__ unsigned long long s_sum[OT_T];
  __shared__ int s_cnt[OT_T];
  __shared__ float s_mx[OT_T];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n4 = n >> 2;
  const uint32_t* lw = reinterpret_cast<const uint32_t*>(labels + (size_t)b * n);
  const float4* dp = reinterpret_cast<const float4*>(depth + (size_t)b * n);
  if (blockIdx.x == OT_LAB) {                                  // the status bits 0, 1, 3 of the room
    int f = 0;
    for (int64_t g = tid; g < n4; g += OT_T) {
      const uint32_t w = lw[g];
      const float4 d4 = dp[g];
      const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned y = (w >> (8 * i)) & 0xffu;
        const bool rd = obs_reading(d[i]);
        if (y > (unsigned)OT_LAB) f |= 1;
        else if (y > 0u) f |= rd ? (((known >> y) & 1ull) ? 0 : 2) : 8;
      }
    }
    s_cnt[tid] = f;
    __syncthreads();
    for (int o = OT_T / 2; o > 0; o >>= 1) {
      if (tid < o) s_cnt[tid] |= s_cnt[tid + o];
      __syncthreads();
    }
    if (tid == 0) { ws[b].flags = s_cnt[0]; ws[b].pad_ = 0; }
    return;
  }
  const unsigned v = blockIdx.x + 1u;                          // this workgroup's label value
  unsigned long long sum = 0ull;
  int cnt = 0;
  float mx = -INFINITY;
  for (int64_t g = tid; g < n4; g += OT_T) {
    const uint32_t w = lw[g];
    const bool hit[4] = {(w & 0xffu) == v, ((w >> 8) & 0xffu) == v, ((w >> 16) & 0xffu) == v, (w >> 24) == v};
    if (!(hit[0] || hit[1] || hit[2] || hit[3])) continue;
    const float4 d4 = dp[g];
    const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (hit[i] && obs_reading(d[i])) {
        sum += (unsigned long long)(long long)rint((double)d[i] * 4294967296.0);
        cnt += 1;
        mx = fmaxf(mx, d[i]);
      }
  }
  s_sum[tid] = sum; s_cnt[tid] = cnt; s_mx[tid] = mx;
  __syncthreads();
  for (int o = OT_T / 2; o > 0; o >>= 1) {
    if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + o]); }
    __syncthreads();
  }
  if (tid == 0) {
    ws[b].sum_lo[v - 1] = (uint32_t)s_sum[0]; ws[b].sum_hi[v - 1] = (uint32_t)(s_sum[0] >> 32);
    ws[b].cnt[v - 1] = s_cnt[0]; ws[b].mx[v - 1] = s_mx[0];
  }
}

__global__ void __launch_bounds__(OT_T) observed_compose(const float* __restrict__ depth, const unsigned char* __restrict__ labels, int64_t n,
                                                        int nch, OtTabs tabs, const OtRoom* __restrict__ ws, float* __restrict__ out,
                                                        int32_t* __restrict__ status) {
  __shared__ int s_own[OT_MAX_DCH + 1];
  __shared__ float s_fill[OT_MAX_DCH + 1];
  __shared__ float s_wall;
  const int b = blockIdx.y, tid = threadIdx.x, ndch = nch - OT_DEP0;
  if (tid <= OT_MAX_DCH) {
    const OtRoom& r = ws[b];
    const int wl = tabs.wall_label;
    const float wall_max = r.cnt[wl - 1] > 0 ? r.mx[wl - 1] : 10.0f;
    const int own = tid < ndch ? tabs.own_label[tid] : 0;
    float fill = 0.f;
    if (own > 0) {
      const int cnt = r.cnt[own - 1];
      const long long isum = (long long)((unsigned long long)r.sum_hi[own - 1] << 32 | r.sum_lo[own - 1]);
      const double sum = (double)isum * (1.0 / 4294967296.0);
      fill = cnt > 0 ? (float)(sum / (double)cnt) : wall_max;
    }
    s_own[tid] = own;
    s_fill[tid] = fill / wall_max;
    if (tid == 0) {
      s_wall = wall_max;
      if (blockIdx.x == 0) status[b] = r.flags | (r.cnt[wl - 1] > 0 ? 0 : 4);
    }
  }
  __syncthreads();
  const int64_t p = ((int64_t)blockIdx.x * OT_T + tid) * 4;
  if (p >= n) return;
  const uint32_t w = *reinterpret_cast<const uint32_t*>(labels + (size_t)b * n + p);
  const float4 d4 = *reinterpret_cast<const float4*>(depth + (size_t)b * n + p);
  const float d[4] = {d4.x, d4.y, d4.z, d4.w};
  const float wall_max = s_wall;
  float d0[4], dq[4];
  int l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned y = (w >> (8 * i)) & 0xffu;
    const bool rd = obs_reading(d[i]);
    d0[i] = rd ? d[i] : -1.f;
    l[i] = (rd && y <= (unsigned)OT_LAB) ? (int)y : 0;
    dq[i] = d0[i] / wall_max;
  }
  float* o = out + (size_t)b * nch * n + p;
  *reinterpret_cast<float4*>(o) = make_float4(d0[0], d0[1], d0[2], d0[3]);
  for (int c = 0; c < OT_LAB; ++c) {
    const int v = c + 1;
    *reinterpret_cast<float4*>(o + (size_t)(OT_SEM0 + c) * n) =
        make_float4(l[0] == v ? 1.f : 0.f, l[1] == v ? 1.f : 0.f, l[2] == v ? 1.f : 0.f, l[3] == v ? 1.f : 0.f);
  }
  for (int k = 0; k < ndch; ++k) {
    const int own = s_own[k];
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (own > 0) {
      const float fq = s_fill[k];
      x = make_float4(l[0] == own ? dq[0] : fq, l[1] == own ? dq[1] : fq, l[2] == own ? dq[2] : fq, l[3] == own ? dq[3] : fq);
    }
    *reinterpret_cast<float4*>(o + (size_t)(OT_DEP0 + k) * n) = x;
  }
}

}  // namespace

extern "C" int64_t sln_observed_target_workspace_bytes(int B, int S) {
  if (S < 4 || S % 4 != 0 || S > OBS_MAX_S || !obs_batch_ok(B)) return SLN_E_UNSUPPORTED;
  return (int64_t)B * (int64_t)sizeof(OtRoom);
}

extern "C" int sln_observed_target(const float* depth, const unsigned char* labels, int B, int S, int NC, const int32_t* chan,
                                   const int32_t* dch, int nch, void* workspace, float* out, int32_t* status, void* stream) {
  if (S < 4 || S % 4 != 0 || S > OBS_MAX_S || !obs_batch_ok(B) || NC < 1 || NC > 64 || nch < OT_DEP0 || nch > OT_DEP0 + OT_MAX_DCH)
    return SLN_E_UNSUPPORTED;
  if (!depth || !labels || !chan || !dch || !workspace || !out || !status) return SLN_E_BADARG;
  int owned = 0;
  for (int c = 0; c < NC; ++c) owned += dch[c] >= 0 ? 1 : 0;
  if (nch != OT_DEP0 + owned) return SLN_E_UNSUPPORTED;
  // float4 loads and stores, 32-bit loads of four label bytes: the bases must allow them (the plane and room strides do, S % 4 == 0)
  if (reinterpret_cast<uintptr_t>(depth) % 16 || reinterpret_cast<uintptr_t>(out) % 16 || reinterpret_cast<uintptr_t>(labels) % 4 ||
      reinterpret_cast<uintptr_t>(workspace) % 4 || reinterpret_cast<uintptr_t>(status) % 4 || reinterpret_cast<uintptr_t>(chan) % 4 ||
      reinterpret_cast<uintptr_t>(dch) % 4)
    return SLN_E_BADARG;
  OtTabs tabs;
  for (int k = 0; k <= OT_MAX_DCH; ++k) tabs.own_label[k] = 0;
  unsigned long long known = 0ull;
  const int ndch = nch - OT_DEP0;
  for (int c = 0; c < NC; ++c) {
    if (chan[c] < 0 || chan[c] >= OT_LAB || dch[c] < -1 || dch[c] >= ndch) return SLN_E_BADARG;
    known |= 1ull << (chan[c] + 1);
    if (dch[c] >= 0) {
      if (tabs.own_label[dch[c]] != 0) return SLN_E_BADARG;               // a depth channel owned twice
      tabs.own_label[dch[c]] = chan[c] + 1;
    }
  }
  tabs.wall_label = chan[0] + 1;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)S * S;
  OtRoom* ws = static_cast<OtRoom*>(workspace);
  hipLaunchKernelGGL(observed_stats, dim3(OT_LAB + 1, B), dim3(OT_T), 0, st, depth, labels, n, known, ws);
  SLN_CHECK_LAUNCH();
  const unsigned G = (unsigned)((n / 4 + OT_T - 1) / OT_T);
  hipLaunchKernelGGL(observed_compose, dim3(G, B), dim3(OT_T), 0, st, depth, labels, n, nch, tabs, ws, out, status);
  SLN_CHECK_LAUNCH();
  return 0;
}
