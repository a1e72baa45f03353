// An observed frame finer than the refinement view, decimated by an integer factor f in front of the reprojection (host/reproject.py:
// ObservedPrefilter; DESIGN §4 "Observed frames finer than the target" and include/sln_hip.h above sln_observed_prefilter are the
// definition).  Coarse pixel (I, J) owns the f x f block of source pixels [f I, f I + f) x [f J, f J + f):
//
//   observed_prefilter_kernel<F>   grid (tiles, B), one wavefront per workgroup: a tile of TW x TH = 32 x 2 coarse pixels of one frame.
//                                  Load: the tile's TH * F source rows of up to TW * F pixels go through LDS.  A row is cut into
//                                  16-byte chunks at the ALIGNED addresses of depth_src; a chunk that lies wholly inside the row's
//                                  valid span is one 16-byte load (four pixels a lane), the chunks on either end - the scalar head
//                                  and tail, Ws being arbitrary - load their valid pixels one by one.  The (row, chunk) pairs of
//                                  the tile are dealt over the 64 lanes.  A depth that is no reading is stored as 0.0f, so LDS
//                                  holds "reading iff > 0".  LDS layout: [i * F + j][lane of the owning coarse pixel] - the 64 lanes
//                                  of the compute phase read consecutive dwords (bytes for the labels): no bank conflict.
//                                  Compute: a lane owns one coarse pixel and reads its n = F * F pixels out of LDS: the count of
//                                  readings; the lower median by building its bit pattern from the top bit down (positive floats
//                                  order as their bits; 31 counting passes, no sort, no per-lane array); the member test against
//                                  it, a 64-bit member mask; the sum of 1.0 / (double)d over the members in row-major order; the
//                                  vote over the members' bytes (a pass per distinct candidate, skipped while the candidate is the
//                                  current best).
//
// k_out: lanes 0 .. 3 of the frame's first workgroup.  counts: ballots and popcounts, one 64-bit integer atomic per workgroup and
// non-zero counter.  No allocation, synchronisation, read-back or floating-point atomic; every index is formed from the launch's own
// sizes - no address depends on data.  Built with -ffp-contract=off: the harmonic mean is a chain of correctly rounded double
// operations; the member test is observed_rules.h's depth-step test, which rounds each operation under either flag.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "observed_rules.h"
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int TW = 32, TH = 2, LANES = TW * TH;   // coarse pixels per workgroup: one wavefront

template <int F>
__global__ __launch_bounds__(LANES) void observed_prefilter_kernel(const float* __restrict__ depth_src, const unsigned char* __restrict__ labels_src,
                                                                   const float* __restrict__ k_src, int Hs, int Ws, int Hd, int Wd, int tiles_x,
                                                                   float gap, float* __restrict__ depth_out, unsigned char* __restrict__ labels_out,
                                                                   float* __restrict__ k_out, unsigned long long* __restrict__ counts) {
  constexpr int N = F * F;
  constexpr int ROWS = TH * F, COLS = TW * F;      // the tile in source pixels
  constexpr int NCH = COLS / 4 + 1;                // 16-byte chunks a row of COLS floats can touch
  __shared__ float sd[N * LANES];
  __shared__ unsigned char sl[N * LANES];
  const int lane = threadIdx.x;
  const int b = blockIdx.y;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  if (blockIdx.x == 0 && lane < 4) k_out[4 * b + lane] = __fdiv_rn(k_src[4 * b + lane], (float)F);

  // ---- load: rows [r0, r0 + rows) x columns [c0, c0 + cols) of frame b, all inside [0, F Hd) x [0, F Wd)
  const int r0 = tile_y * ROWS, c0 = tile_x * COLS;
  const int rows = min(ROWS, F * Hd - r0), cols = min(COLS, F * Wd - c0);
  const long frame = (long)b * Hs * Ws;
  for (int e = lane; e < rows * NCH; e += LANES) {
    const int r = e / NCH, s = e - r * NCH;
    const long at = frame + (long)(r0 + r) * Ws + c0;                // the row's first pixel
    const float* row_d = depth_src + at;
    const unsigned char* row_l = labels_src + at;
    const int mis = (int)((reinterpret_cast<uintptr_t>(row_d) >> 2) & 3);   // floats past the 16-byte boundary below the row's start
    const int c = 4 * s - mis;                                       // the chunk's first column in the tile; may be < 0 or reach past cols
    float d[4];
    unsigned char l[4];
    const bool whole = c >= 0 && c + 4 <= cols;
    if (whole) {
      const float4 q = *reinterpret_cast<const float4*>(row_d + c);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool in = c + t >= 0 && c + t < cols;
      if (!whole) d[t] = in ? row_d[c + t] : 0.f;
      l[t] = in ? row_l[c + t] : (unsigned char)0;
    }
    const int ty = r / F, i = r - ty * F;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cc = c + t;
      if (cc < 0 || cc >= cols) continue;
      const int tx = cc / F, j = cc - tx * F;
      const int to = (i * F + j) * LANES + ty * TW + tx;
      // obs_reading(d[t]), spelled out: through the helper hipcc selects on the inverted condition - other code for the same work,
      // which would have to be timed again; written here the kernels keep their code (LAB_NOTES §37)
      sd[to] = (d[t] > 0.f && d[t] <= OBS_FAR) ? d[t] : 0.f;
      sl[to] = l[t];
    }
  }
  __syncthreads();

  // ---- compute: lane (ty, tx) owns coarse pixel (I, J)
  const int I = tile_y * TH + lane / TW, J = tile_x * TW + (lane & (TW - 1));
  const bool live = I < Hd && J < Wd;
  int m = 0, r = 0;
  if (live) {
    const float* my_d = sd + lane;
    const unsigned char* my_l = sl + lane;
#pragma unroll
    for (int t = 0; t < N; ++t) r += my_d[t * LANES] > 0.f ? 1 : 0;
    float z = 0.f;
    unsigned char lab = 0;
    if (2 * r >= N) {
      // the lower median of the readings: rank (r - 1) / 2 among them, rank k among all N values, the N - r zeros first.  The largest
      // bit pattern v with #(values < v) <= k is that value.
      const int k = (r - 1) / 2 + (N - r);
      unsigned v = 0;
      for (int bit = 30; bit >= 0; --bit) {
        const unsigned trial = v | (1u << bit);
        int below = 0;
#pragma unroll
        for (int t = 0; t < N; ++t) below += __float_as_uint(my_d[t * LANES]) < trial ? 1 : 0;
        if (below <= k) v = trial;
      }
      const float dref = __uint_as_float(v);
      unsigned long long member = 0;
      double sum = 0.0;
#pragma unroll
      for (int t = 0; t < N; ++t) {
        const float d = my_d[t * LANES];
        if (!(d > 0.f)) continue;
        const float hi = fmaxf(d, dref), lo = fminf(d, dref);
        if (obs_depth_step(hi, lo, gap)) continue;                   // another surface
        member |= 1ull << t;
        sum += 1.0 / (double)d;
        ++m;
      }
      z = (float)((double)m / sum);
      int best = 0;
      for (int t = 0; t < N; ++t) {
        if (!((member >> t) & 1)) continue;
        const unsigned char a = my_l[t * LANES];
        if (best > 0 && a == lab) continue;                          // counted already
        int n_a = 0;
#pragma unroll
        for (int u = 0; u < N; ++u) n_a += ((member >> u) & 1) && my_l[u * LANES] == a ? 1 : 0;
        if (n_a > best || (n_a == best && a < lab)) { best = n_a; lab = a; }
      }
    }
    const long q = ((long)b * Hd + I) * Wd + J;
    depth_out[q] = z;
    labels_out[q] = lab;
  }
  if (counts) {
    const int full = __popcll(__ballot(live && m == N));
    const int mixed = __popcll(__ballot(live && m > 0 && m < N));
    const int none = __popcll(__ballot(live && m == 0));
    if (lane == 0) {                                                 // (integers: the totals do not depend on the order)
      if (full) atomicAdd(counts + 3 * b + 0, (unsigned long long)full);
      if (mixed) atomicAdd(counts + 3 * b + 1, (unsigned long long)mixed);
      if (none) atomicAdd(counts + 3 * b + 2, (unsigned long long)none);
    }
  }
}

template <int F>
void launch(dim3 grid, hipStream_t st, const float* depth_src, const unsigned char* labels_src, const float* k_src, int Hs, int Ws, int Hd, int Wd,
            int tiles_x, float gap, float* depth_out, unsigned char* labels_out, float* k_out, unsigned long long* counts) {
  hipLaunchKernelGGL(observed_prefilter_kernel<F>, grid, dim3(LANES), 0, st, depth_src, labels_src, k_src, Hs, Ws, Hd, Wd, tiles_x, gap, depth_out,
                     labels_out, k_out, counts);
}

}  // namespace

extern "C" {

int sln_observed_prefilter(const float* depth_src, const unsigned char* labels_src, const float* k_src, int B, int Hs, int Ws, int f, float gap,
                           float* depth_out, unsigned char* labels_out, float* k_out, int64_t* counts, void* stream) {
  if (!depth_src || !labels_src || !k_src || !depth_out || !labels_out || !k_out) return SLN_E_BADARG;
  if (!obs_batch_ok(B) || f < 1 || f > OBS_MAX_PREFILTER || Hs < f || Ws < f) return SLN_E_BADARG;
  if (!(gap >= 0.f)) return SLN_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(counts) & 7) || (reinterpret_cast<uintptr_t>(depth_out) & 3) || (reinterpret_cast<uintptr_t>(depth_src) & 3) ||
      (reinterpret_cast<uintptr_t>(k_src) & 3) || (reinterpret_cast<uintptr_t>(k_out) & 3))
    return SLN_E_BADARG;
  const int Hd = Hs / f, Wd = Ws / f;
  const long tiles_x = (Wd + TW - 1) / TW, tiles_y = (Hd + TH - 1) / TH;
  if (tiles_x * tiles_y > 0x7fffffffL) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (counts) {
    const int e = sln_zero_async(counts, sizeof(int64_t) * 3 * (size_t)B, st);
    if (e != 0) return e;
  }
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B);
  unsigned long long* cn = reinterpret_cast<unsigned long long*>(counts);
#define SLN_PREFILTER_CASE(F) \
  case F: launch<F>(grid, st, depth_src, labels_src, k_src, Hs, Ws, Hd, Wd, (int)tiles_x, gap, depth_out, labels_out, k_out, cn); break;
  switch (f) {
    SLN_PREFILTER_CASE(1) SLN_PREFILTER_CASE(2) SLN_PREFILTER_CASE(3) SLN_PREFILTER_CASE(4)
    SLN_PREFILTER_CASE(5) SLN_PREFILTER_CASE(6) SLN_PREFILTER_CASE(7) SLN_PREFILTER_CASE(8)
  }
#undef SLN_PREFILTER_CASE
  SLN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
