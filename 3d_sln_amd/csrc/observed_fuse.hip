// Several observed frames per room, fused into one refinement target (host/reproject.py: ObservedFuser; DESIGN §4 "Several observed
// frames per room" and include/sln_hip.h above sln_reproject_fuse are the definition).  The V frames of a room are reprojected and drawn
// as B = R * V separate frames (observed_reproject.hip, sln_raster_forward); this unit decides, per target pixel, which of them the
// target view sees:
//
//   reproject_fuse_kernel      grid (pixel blocks, R): a lane owns one target pixel of one room.  Pass 1 walks v upwards with the
//                              face_index and depth loads of four frames in flight and carries (dmin, v*): a candidate whose index lies in
//                              [0, F), whose depth is no NaN and which would become the best (none yet, or d < dmin: strict, so equal
//                              depths stay with the lower v) has its three weights loaded and NaN-checked - the weights of the winner are
//                              the last ones that passed, so they are never loaded twice; a candidate that could not win has its weights
//                              untouched in this pass.  Compose for the winner alone: corner of largest weight, label byte gathered, depth
//                              bits copied - no per-frame depth / label intermediates.  Pass 2 runs only where count_out or agree_out is
//                              asked for and the pixel has a winner: the V depths are read again (L1 / L2), and because `count` and
//                              `agree` are defined over CONTRIBUTING frames the weights of every in-range candidate other than the
//                              winner are loaded here for the NaN rule - the one place a losing frame's weights are read.
//
// hits: observed_rules.h's workgroup count, as reproject_compose_kernel; so are the hit rule and the label gather.  wins: an LDS array of V
// integer counters per workgroup, one 64-bit integer atomic per non-zero counter.  Integer sums only: the same from call to call.  No
// allocation, synchronisation, read-back or floating-point atomic.  Every index read from a map is compared with its range before it
// addresses anything.  The agreement test is the face kernel's depth-step test (observed_rules.h: one rounded difference against one
// rounded product, which contraction cannot fuse); everything else copies bits and bytes, so the unit takes the default flags.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "observed_rules.h"
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int IN_FLIGHT = 4;               // frames whose face_index and depth are loaded before the first of them is looked at

__global__ __launch_bounds__(256) void reproject_fuse_kernel(const int32_t* __restrict__ fi, const float* __restrict__ weight,
                                                             const float* __restrict__ depth, const unsigned char* __restrict__ labels_src,
                                                             int V, int Hs, int Ws, int S, float gap, float* __restrict__ dout,
                                                             unsigned char* __restrict__ lout, unsigned char* __restrict__ src,
                                                             unsigned char* __restrict__ cnt, unsigned char* __restrict__ agr,
                                                             unsigned long long* __restrict__ hits, unsigned long long* __restrict__ wins) {
  __shared__ int wcnt[OBS_MAX_VIEWS + 1];
  const int r = blockIdx.y;
  const long n = (long)S * S;
  const long room = (long)r * V * n;                               // the room's first frame in the maps
  const int F = obs_n_faces(Hs, Ws);
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (wins)
    for (int v = threadIdx.x; v < V; v += 256) wcnt[v] = 0;
  __syncthreads();
  int best = -1;
  if (p < n) {
    const int y = (int)(p / S), x = (int)(p - (long)y * S);
    float dmin = 0.f, w0 = 0.f, w1 = 0.f, w2 = 0.f;
    int kbest = 0;
    for (int v0 = 0; v0 < V; v0 += IN_FLIGHT) {
      int k[IN_FLIGHT];
      float d[IN_FLIGHT];
#pragma unroll
      for (int j = 0; j < IN_FLIGHT; ++j) {
        const bool live = v0 + j < V;
        const long at = room + (long)(v0 + j) * n + p;
        k[j] = live ? fi[at] : -1;
        d[j] = live ? depth[at] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < IN_FLIGHT; ++j) {
        if (!obs_face_in_range(k[j], F) || d[j] != d[j]) continue;
        if (best >= 0 && !(d[j] < dmin)) continue;                 // strict: equal depths stay with the lower v
        const float* w = weight + 3 * (room + (long)(v0 + j) * n + p);
        const float a = w[0], b = w[1], c = w[2];
        if (obs_any_nan(a, b, c)) continue;                        // not a hit: the previous best stands
        best = v0 + j; dmin = d[j]; kbest = k[j]; w0 = a; w1 = b; w2 = c;
      }
    }
    unsigned char lab = 0;
    float z = -1.0f;
    int count = 0, agree = 0;
    if (best >= 0) {
      lab = labels_src[obs_label_index((long)r * V + best, kbest, w0, w1, w2, Hs, Ws)];
      z = dmin;
      if (cnt || agr) {
        const float edge = obs_step_edge(gap, dmin);
        for (int v0 = 0; v0 < V; v0 += IN_FLIGHT) {
          int k[IN_FLIGHT];
          float d[IN_FLIGHT];
#pragma unroll
          for (int j = 0; j < IN_FLIGHT; ++j) {
            const bool live = v0 + j < V;
            const long at = room + (long)(v0 + j) * n + p;
            k[j] = live ? fi[at] : -1;
            d[j] = live ? depth[at] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < IN_FLIGHT; ++j) {
            if (!obs_face_in_range(k[j], F) || d[j] != d[j]) continue;
            if (v0 + j != best) {                                  // the NaN rule of a candidate that did not win
              const float* w = weight + 3 * (room + (long)(v0 + j) * n + p);
              if (obs_any_nan(w[0], w[1], w[2])) continue;
            }
            ++count;
            agree += !(obs_step_rise(d[j], dmin) > edge) ? 1 : 0;
          }
        }
      }
    }
    const long q = (long)r * n + (long)(S - 1 - y) * S + x;        // the planes' rows run downwards
    dout[q] = z;
    lout[q] = lab;
    if (src) src[q] = (unsigned char)(best + 1);
    if (cnt) cnt[q] = (unsigned char)count;
    if (agr) agr[q] = (unsigned char)agree;
    if (wins && best >= 0) atomicAdd(&wcnt[best], 1);
  }
  obs_count_flags(best >= 0, hits + r);                            // (its barrier also orders the wcnt updates before the reads below)
  if (wins)
    for (int v = threadIdx.x; v < V; v += 256)
      if (wcnt[v]) atomicAdd(wins + (long)r * V + v, (unsigned long long)wcnt[v]);
}

}  // namespace

extern "C" {

int sln_reproject_fuse(const int32_t* face_index, const float* weight, const float* raster_depth, const unsigned char* labels_src, int R,
                       int V, int Hs, int Ws, int S, float gap, float* depth_out, unsigned char* labels_out, unsigned char* source_out,
                       unsigned char* count_out, unsigned char* agree_out, int64_t* hits, int64_t* wins, void* stream) {
  if (!face_index || !weight || !raster_depth || !labels_src || !depth_out || !labels_out || !hits) return SLN_E_BADARG;
  if (R < 1 || !obs_views_ok(V) || obs_check_frames((long)R * V, Hs, Ws) || !obs_target_ok(S)) return SLN_E_BADARG;
  if (!(gap >= 0.f)) return SLN_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(hits) & 7) || (reinterpret_cast<uintptr_t>(wins) & 7) || (reinterpret_cast<uintptr_t>(depth_out) & 3))
    return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  int e = sln_zero_async(hits, sizeof(int64_t) * (size_t)R, st);
  if (e != 0) return e;
  if (wins) {
    e = sln_zero_async(wins, sizeof(int64_t) * (size_t)R * (size_t)V, st);
    if (e != 0) return e;
  }
  const long n = (long)S * S;
  hipLaunchKernelGGL(reproject_fuse_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)R), dim3(256), 0, st, face_index, weight, raster_depth,
                     labels_src, V, Hs, Ws, S, gap, depth_out, labels_out, source_out, count_out, agree_out,
                     reinterpret_cast<unsigned long long*>(hits), reinterpret_cast<unsigned long long*>(wins));
  SLN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
