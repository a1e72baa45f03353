// The rules the steps of the observed-frame route share (DESIGN §4 "One home for the rules of the observed-frame route"): what a
// reading is, what a depth step is, which source pixel a rasterizer hit takes its label from, how a workgroup counts its hits, and the
// sizes the entry points accept.  observed_target.hip, observed_prefilter.hip, observed_reproject.hip and observed_fuse.hip include it
// and stay translation units of their own (build.py gives them different contraction flags); host/reproject.py restates the same rules
// in torch ops once (_reading, _hit_and_label, _check_sizes).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sln_hip.h"

// ---- a reading: 0 < d <= 15 (host/observe.py: FAR); a NaN, an infinity, d <= 0 and d > 15 are none
constexpr float OBS_FAR = 15.0f;
__device__ __forceinline__ bool obs_reading(float d) { return d > 0.f && d <= OBS_FAR; }

// ---- a depth step: hi - lo > gap * lo, ONE rounded difference against ONE rounded product (contraction cannot fuse them: the bits are
// those of torch's float32 subtraction and multiplication under either contraction flag).  The two halves are functions of their own
// for a caller that tests many `hi` against one `lo` and keeps the product: rise > edge.  (The difference is formed first: with the
// product first the face kernel is scheduled differently and takes one VGPR more, LAB_NOTES §37.)
__device__ __forceinline__ float obs_step_rise(float hi, float lo) { return __fsub_rn(hi, lo); }
__device__ __forceinline__ float obs_step_edge(float gap, float lo) { return __fmul_rn(gap, lo); }
__device__ __forceinline__ bool obs_depth_step(float hi, float lo, float gap) { return obs_step_rise(hi, lo) > obs_step_edge(gap, lo); }

// ---- a hit of one frame, and the pixel its label comes from.  A frame of Hs x Ws pixels is a mesh of (Hs - 1) x (Ws - 1) cells with
// corners a (0, 0), b (1, 0), c (0, 1), d (1, 1) (row, column); cell e gives the faces 2 e: (a, b, c) and 2 e + 1: (d, c, b).  A map
// entry is a hit when its face index lies in [0, F) and none of its three weights is a NaN; the label is that of the corner of largest
// weight, ties to the lower corner number.  The parts are separate so that a caller may test the index before it loads the weights.
__host__ __device__ __forceinline__ int obs_n_faces(int Hs, int Ws) { return 2 * (Hs - 1) * (Ws - 1); }
__device__ __forceinline__ bool obs_face_in_range(int k, int F) { return k >= 0 && k < F; }
__device__ __forceinline__ bool obs_any_nan(float a, float b, float c) { return a != a || b != b || c != c; }
__device__ __forceinline__ bool obs_hit(int k, int F, float w0, float w1, float w2) { return obs_face_in_range(k, F) && !obs_any_nan(w0, w1, w2); }
// the index into labels_src [frames, Hs, Ws] of the label of face k (in [0, F): the cell lies inside the frame) of frame `frame`
__device__ __forceinline__ long obs_label_index(long frame, int k, float w0, float w1, float w2, int Hs, int Ws) {
  int corner = w1 > w0 ? 1 : 0;
  if (w2 > (corner ? w1 : w0)) corner = 2;
  const int Wc = Ws - 1, cell = k >> 1, which = k & 1;
  const int ci = cell / Wc, cj = cell - ci * Wc;
  const int di = which ? (corner == 1 ? 0 : 1) : (corner == 1 ? 1 : 0);
  const int dj = which ? (corner == 2 ? 0 : 1) : (corner == 2 ? 1 : 0);
  return (frame * Hs + ci + di) * Ws + cj + dj;
}

// ---- one flag per lane of a workgroup of 256 -> `total`: ballot and popcount per wavefront, one 64-bit integer atomic per workgroup
// with a non-zero count (integers: the total does not depend on the order).  Every lane of the workgroup calls it, once.
__device__ __forceinline__ void obs_count_flags(bool flag, unsigned long long* total) {
  __shared__ int red[4];
  const int c = __popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(total, (unsigned long long)s);
  }
}

// ---- the sizes the entry points accept (include/sln_hip.h): frames ride gridDim.y; `source` is a byte, 1 + v; F is sln_raster_forward's
constexpr int OBS_MAX_FRAMES = 65535, OBS_MAX_S = 4096, OBS_MAX_VIEWS = 255, OBS_MAX_PREFILTER = 8;
constexpr long OBS_MAX_FACES = 1L << 24;
static inline bool obs_batch_ok(long B) { return B >= 1 && B <= OBS_MAX_FRAMES; }
static inline bool obs_target_ok(int S) { return S >= 1 && S <= OBS_MAX_S; }
static inline bool obs_views_ok(int V) { return V >= 1 && V <= OBS_MAX_VIEWS; }
// B frames that the face step can mesh: at least 2 x 2 pixels, at most 2^24 faces each
static inline int obs_check_frames(long B, int Hs, int Ws) {
  if (!obs_batch_ok(B) || Hs < 2 || Ws < 2) return SLN_E_BADARG;
  if (2L * (Hs - 1) * (Ws - 1) > OBS_MAX_FACES) return SLN_E_BADARG;
  return 0;
}
