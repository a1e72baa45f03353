// Refinement loss of the layout-refinement loop (testing/test_render_refine.py:192-215 PSP_pool_new, :332-356 the loss):
//
//   iter[:, -1][sum(iter[:, 41:], 1) < 0.5] = 1                                   null regions
//   depth = L1( cat_s pool_s(iter[:, 41:]), cat_s pool_s(target[:, 41:]) ) * 0.5   pool_s = bilinear(align_corners) to s x s,
//   sem   = sum_s CE( pool_s(iter[:, 1:41]), argmax labels of the target ) / 800            then bilinear to 96 x 96
//   loss  = 100 * depth + 100 * sem  (+ 2 * size_loss, added by the caller)
//
// In torch this is ~200 small launches per iteration (16 resamples forward and backward, softmax / nll per scale, fills, cats)
// and was 60 % of a refinement iteration.  Here: null mask, one resampling kernel for the 4 scales x 69 channels (both
// interpolation stages in registers, same order of operations as upsample_bilinear2d), one loss kernel that leaves
// d loss / d pooled in place of the pooled maps, and for backward ONE gather kernel through the transposed resampling
// operator (a bilinear DOWN-sample without anti-aliasing reads few input pixels, so the image gradient is sparse; every
// input pixel sums the few pooled pixels that read it - no atomics).  The target's pooled depth maps and labels are
// constants of a room; the host derives them from sln_refine_pool of the target (the same resampling kernel).
//
// Three routes through the loss, finalize and report kernels, chosen by the descriptor: unmasked; under a validity mask of the target
// (valid_pooled / valid_image / depth_count, set up by sln_refine_loss_mask); under a per-pixel confidence of the target (the same
// fields holding bytes 0..255 plus conf_sum, set up by sln_refine_loss_confidence: a pooled pixel weighs c / 255, every mean is divided
// by the sum of its weights).  A {0, 255} confidence gives the masked route's bits, all 255 the unmasked route's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int MAX_SCALES = 4;

struct RefineDims {
  int B, S, P, C;                 // batch, image size, pooled size, image channels (70)
  int sem0, n_sem, dep0, n_dep;   // semantic channels [sem0, sem0 + n_sem), depth channels [dep0, dep0 + n_dep) (contiguous)
  int n_scales, pmax;             // pmax: row length of the stage-1 tables (largest intermediate size)
  int per_room, pad_;             // per_room: B independent rooms - every room's loss is normalised by its OWN element / label counts
};

// `live` (SlnRefineLoss::live_planes): a plane marked 0 is all zeros, a plane marked 1 the constant 1 - the same sum without the load
__global__ void null_mask_kernel(const float* __restrict__ img, RefineDims d, unsigned char* __restrict__ null,
                                 const unsigned char* __restrict__ live) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long plane = (long)d.S * d.S;
  if (i >= d.B * plane) return;
  const long b = i / plane, pix = i % plane;
  const float* p = img + (b * d.C + d.dep0) * plane + pix;
  float s = 0.f;
  if (live != nullptr) {
    const unsigned char* lv = live + b * d.C + d.dep0;
    for (int c = 0; c < d.n_dep; ++c) { const int k = lv[c]; s += k == 3 ? p[c * plane] : (k == 1 ? 1.f : 0.f); }
  } else
  for (int c = 0; c < d.n_dep; ++c) s += p[c * plane];
  null[i] = s < 0.5f ? 1 : 0;
}

// w0 * a + w1 * b of a bilinear stage with its one fused multiply-add spelled out.  Both pooling kernels form every sample through this
// function: left to the compiler's contraction, pool_kernel and pool_lds_kernel - and the packed and the scalar copy of one loop -
// fused different halves of the sum and differed in the last bit of a third of their outputs (tests/test_refine_loss_family_gpu.py).
__device__ __forceinline__ float lerp2(const float w0, const float a, const float w1, const float b) { return fmaf(w0, a, w1 * b); }
// upsample_bilinear2d's expression h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)
__device__ __forceinline__ float bilerp(const float h0, const float h1, const float w0, const float w1, const float v00, const float v01,
                                        const float v10, const float v11) {
  return lerp2(h0, lerp2(w0, v00, w1, v01), h1, lerp2(w0, v10, w1, v11));
}

// pooled[b][s][cc][oy][ox], cc = channel - sem0 over the n_sem + n_dep loss channels.  One thread resamples one pooled pixel
// of CG consecutive channels: the 12 table entries that locate its 16 taps are loaded once per thread, not once per channel.
constexpr int CG = 8;
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ img, const unsigned char* __restrict__ null, const int null_fill,
                                                   RefineDims d,
                                                   const int* __restrict__ s2_k0, const int* __restrict__ s2_k1, const float* __restrict__ s2_l1,
                                                   const int* __restrict__ s1_i0, const int* __restrict__ s1_i1, const float* __restrict__ s1_l1,
                                                   float* __restrict__ pooled) {
  const int nc = d.n_sem + d.n_dep, ng = (nc + CG - 1) / CG;
  const long pp = (long)d.P * d.P;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)d.B * d.n_scales * ng * pp) return;
  const int ox = (int)(i % d.P), oy = (int)((i / d.P) % d.P);
  const int cg = (int)((i / pp) % ng), s = (int)((i / (pp * ng)) % d.n_scales), b = (int)(i / (pp * ng * d.n_scales));
  const long plane = (long)d.S * d.S;
  const int ky[2] = {s2_k0[s * d.P + oy], s2_k1[s * d.P + oy]}, kx[2] = {s2_k0[s * d.P + ox], s2_k1[s * d.P + ox]};
  const float ly1 = s2_l1[s * d.P + oy], lx1 = s2_l1[s * d.P + ox], ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  int yy[2][2], xx[2][2]; float hh[2], ww[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    yy[a][0] = s1_i0[s * d.pmax + ky[a]]; yy[a][1] = s1_i1[s * d.pmax + ky[a]]; hh[a] = s1_l1[s * d.pmax + ky[a]];
    xx[a][0] = s1_i0[s * d.pmax + kx[a]]; xx[a][1] = s1_i1[s * d.pmax + kx[a]]; ww[a] = s1_l1[s * d.pmax + kx[a]];
  }
  const unsigned char* nm = null + (long)b * plane;
  float* dst = pooled + ((long)(b * d.n_scales + s) * nc) * pp + (long)oy * d.P + ox;
  for (int cc = cg * CG; cc < min(cg * CG + CG, nc); ++cc) {
    const int c = d.sem0 + cc;
    const bool fill = null_fill && c == d.dep0 + d.n_dep - 1;       // the last depth channel is set to 1 where no class has depth
    const float* src = img + ((long)b * d.C + c) * plane;
    float inter[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int y0 = yy[a][0], y1 = yy[a][1];
      const float h1 = hh[a], h0 = 1.f - h1;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int x0 = xx[e][0], x1 = xx[e][1];
        const float w1 = ww[e], w0 = 1.f - w1;
        float v00 = src[(long)y0 * d.S + x0], v01 = src[(long)y0 * d.S + x1], v10 = src[(long)y1 * d.S + x0], v11 = src[(long)y1 * d.S + x1];
        if (fill) {
          v00 = nm[(long)y0 * d.S + x0] ? 1.f : v00; v01 = nm[(long)y0 * d.S + x1] ? 1.f : v01;
          v10 = nm[(long)y1 * d.S + x0] ? 1.f : v10; v11 = nm[(long)y1 * d.S + x1] ? 1.f : v11;
        }
        inter[a][e] = bilerp(h0, h1, w0, w1, v00, v01, v10, v11);
      }
    }
    dst[(long)cc * pp] = bilerp(ly0, ly1, lx0, lx1, inter[0][0], inter[0][1], inter[1][0], inter[1][1]);
  }
}

// The same resampling with the INTERMEDIATE image of a (plane, scale) in LDS (round 5): one workgroup per (image b, loss channel,
// scale).  Phase A evaluates the align_corners=True stage once per intermediate pixel (4 image taps each: sz^2 evaluations instead of
// the 4 P^2 the per-pixel kernel above repeats - 16 640 against 147 456 per plane over the four scales), phase B the second stage
// from LDS with coalesced stores.  Same expressions (bilerp), same order: the results are bit-identical to pool_kernel's.  With 16 rooms in
// flight pool_kernel was the largest kernel of a refinement iteration (510 us: 680 M scattered 4-byte taps).
constexpr int POOL_LDS_MAX = 96;
__global__ __launch_bounds__(256) void pool_lds_kernel(const float* __restrict__ img, const unsigned char* __restrict__ null, const int null_fill,
                                                       RefineDims d,
                                                       const int* __restrict__ s2_k0, const int* __restrict__ s2_k1, const float* __restrict__ s2_l1,
                                                       const int* __restrict__ s1_i0, const int* __restrict__ s1_i1, const float* __restrict__ s1_l1,
                                                       float* __restrict__ pooled, const unsigned char* __restrict__ live, const int skip_ones) {
  __shared__ float inter[POOL_LDS_MAX * POOL_LDS_MAX];
  const int nc = d.n_sem + d.n_dep;
  // (planes x scales grid.  Round 5 tried the four scale-workgroups of a plane on one XCD, adjacent in launch order, so that the
  //  plane is read from HBM once: 280 us against 223 - the scales differ 9x in work and interleaving them unbalances the XCDs)
  // the scales' workgroups differ 9x in work (intermediate images of 32^2 .. 96^2 pixels) and workgroups are dispatched in block order:
  // the largest scale first (round 6: 76 -> 62 us with 16 rooms in flight)
  const int cc = blockIdx.x % nc, b = blockIdx.x / nc, s = d.n_scales - 1 - (int)blockIdx.y;
  const int c = d.sem0 + cc;
  const int lv = live != nullptr ? live[b * d.C + c] : 3;
  if (!(lv & 1)) {                                                // an all-zero plane: its pooled plane is zero (what the taps would give)
    if (cc < d.n_sem) return;                                     // ... and loss_kernel does not read the dead semantic planes at all
    float* dz = pooled + ((long)(b * d.n_scales + s) * nc + cc) * ((long)d.P * d.P);
    for (int o = threadIdx.x; o < d.P * d.P; o += 256) dz[o] = 0.f;
    return;
  }
  const bool ones = lv == 1;                                      // the constant 1: the same expressions on 1.f instead of the four taps
  if (ones && skip_ones) return;                                  // ... or not at all: loss_kernel takes the pooled constant plane from pooled_ones
  const int sz = s2_k1[s * d.P + d.P - 1] + 1;                    // intermediate size of this scale (the last pooled index reads its last row)
  const long plane = (long)d.S * d.S;
  const bool fill = null_fill && c == d.dep0 + d.n_dep - 1;       // the last depth channel is set to 1 where no class has depth
  const float* src = img + ((long)b * d.C + c) * plane;
  const unsigned char* nm = null + (long)b * plane;
  for (int i = threadIdx.x; i < sz * sz; i += 256) {
    const int ky = i / sz, kx = i % sz;
    const int y0 = s1_i0[s * d.pmax + ky], y1 = s1_i1[s * d.pmax + ky], x0 = s1_i0[s * d.pmax + kx], x1 = s1_i1[s * d.pmax + kx];
    const float h1 = s1_l1[s * d.pmax + ky], h0 = 1.f - h1, w1 = s1_l1[s * d.pmax + kx], w0 = 1.f - w1;
    float v00 = 1.f, v01 = 1.f, v10 = 1.f, v11 = 1.f;
    if (!ones) { v00 = src[(long)y0 * d.S + x0]; v01 = src[(long)y0 * d.S + x1]; v10 = src[(long)y1 * d.S + x0]; v11 = src[(long)y1 * d.S + x1]; }
    if (fill) {
      v00 = nm[(long)y0 * d.S + x0] ? 1.f : v00; v01 = nm[(long)y0 * d.S + x1] ? 1.f : v01;
      v10 = nm[(long)y1 * d.S + x0] ? 1.f : v10; v11 = nm[(long)y1 * d.S + x1] ? 1.f : v11;
    }
    inter[i] = bilerp(h0, h1, w0, w1, v00, v01, v10, v11);
  }
  __syncthreads();
  float* dst = pooled + ((long)(b * d.n_scales + s) * nc + cc) * ((long)d.P * d.P);
  for (int o = threadIdx.x; o < d.P * d.P; o += 256) {
    const int oy = o / d.P, ox = o % d.P;
    const int ky0 = s2_k0[s * d.P + oy], ky1 = s2_k1[s * d.P + oy], kx0 = s2_k0[s * d.P + ox], kx1 = s2_k1[s * d.P + ox];
    const float ly1 = s2_l1[s * d.P + oy], lx1 = s2_l1[s * d.P + ox], ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    dst[o] = bilerp(ly0, ly1, lx0, lx1, inter[ky0 * sz + kx0], inter[ky0 * sz + kx1], inter[ky1 * sz + kx0], inter[ky1 * sz + kx1]);
  }
}

// one thread per pooled pixel of one scale and part (blockIdx.y: 0 = log-softmax / NLL over the semantic channels, 1.. = |.| over
// DCH depth channels); overwrites pooled with d loss / d pooled.  partial = per-block {sum |diff|, sum_s CE_s / 800 / valid count}.
//
// MASKED (SlnRefineLoss::valid_pooled): the depth part of an invalid pooled pixel forms no difference - its target is not loaded, it
// adds nothing to the partial and stores a gradient of exactly 0 (a branch, not a product with 0: the target may hold NaN there) -
// and gd comes from the room's count of valid pooled pixels (depth_count) instead of the closed form; one mask byte per lane, loaded
// once in front of the channel loops.  The semantic part needs nothing: sln_refine_loss_mask has set the labels to -100.  The
// unmasked instantiation is the kernel of before.
//
// MODE 2, per-pixel confidence (SlnRefineLoss::conf_sum): valid_pooled holds the pooled confidence byte c, w = (float)c / 255.f.  The
// depth part sums w * |diff| and stores +-(gd * w), gd from the room's pooled sum of c (conf_sum row 0) / 255 in place of N; the
// semantic part scales the pixel's k by w (sln_refine_loss_confidence has set the labels under c == 0 to -100 and put the sum of
// c / 255 over the kept labels into inv_count).  c == 0 is selected away as on the masked route.  With every c in {0, 255} w is
// exactly 1.f, (double)(255 N) / 255.0 exactly N and a product with 1.f exact under either contraction: the bits of MODE 1.
constexpr int DCH = 8;               // depth channels per thread of loss_kernel's parts 1..
constexpr int LOSS_PLAIN = 0, LOSS_MASKED = 1, LOSS_CONF = 2;
template <int NSEM, int MODE>
__global__ __launch_bounds__(128) void loss_kernel(float* __restrict__ pooled, RefineDims d, const float* __restrict__ tgt_depth,
                                                   const int* __restrict__ labels, const float* __restrict__ inv_count,
                                                   float2* __restrict__ partial, const unsigned char* __restrict__ live,
                                                   const float* __restrict__ pooled_ones, const unsigned char* __restrict__ valid_pooled,
                                                   const int32_t* __restrict__ depth_count, const int64_t* __restrict__ conf_sum) {
  constexpr bool MASKED = MODE != LOSS_PLAIN, CONF = MODE == LOSS_CONF;
  const int nc = d.n_sem + d.n_dep;
  const long pp = (long)d.P * d.P;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)d.B * d.n_scales * pp;
  float l_abs = 0.f, l_ce = 0.f;
  if (i < total) {
    const long pix = i % pp;
    const int s = (int)((i / pp) % d.n_scales), b = (int)(i / (pp * d.n_scales));
    float* p = pooled + ((long)(b * d.n_scales + s) * nc) * pp + pix;
    if (blockIdx.y == 0) {
      const int t = labels[i];
      // semantic planes marked all-zero (live_planes) enter as the zeros they are, unread (pool_lds_kernel did not write them), and
      // their gradient, which nobody reads, is not stored
      unsigned long long lm = ~0ull;
      if (live != nullptr) {
        lm = 0;
        const unsigned char* lv = live + b * d.C + d.sem0;
        for (int c = 0; c < NSEM; ++c) lm |= (unsigned long long)(lv[c] & 1) << c;
      }
      float v[NSEM];
#pragma unroll
      for (int c = 0; c < NSEM; ++c) v[c] = (lm >> c & 1) ? p[c * pp] : 0.f;
      if (t >= 0) {
        float m = v[0];
#pragma unroll
        for (int c = 1; c < NSEM; ++c) m = fmaxf(m, v[c]);
        float z = 0.f;
#pragma unroll
        for (int c = 0; c < NSEM; ++c) z += expf(v[c] - m);
        const float lse = m + logf(z);
        float k = inv_count[d.per_room ? b * d.n_scales + s : s] * (1.f / 800.f);
        if (CONF) k *= (float)valid_pooled[i] / 255.f;                              // kw = k * w (a kept label has c > 0)
        float vt = 0.f;
#pragma unroll
        for (int c = 0; c < NSEM; ++c) {
          vt = c == t ? v[c] : vt;
          if (lm >> c & 1) p[c * pp] = (expf(v[c] - lse) - (c == t ? 1.f : 0.f)) * (k * 100.f);
        }
        l_ce = (lse - vt) * k;
      } else {
#pragma unroll
        for (int c = 0; c < NSEM; ++c) if (lm >> c & 1) p[c * pp] = 0.f;
      }
    } else {                                                                       // depth channels, DCH per thread
      float gd = 50.f / (float)((double)(d.per_room ? 1 : d.B) * d.n_scales * d.n_dep * pp);      // 100 * 0.5 / numel
      bool ok = true;
      if (MASKED) {                                                                 // numel = n_dep * N, N the valid pooled pixels (0: no depth term)
        const int nv = depth_count[b];
        gd = nv > 0 ? 50.f / (float)((double)d.n_dep * nv) : 0.f;
        ok = valid_pooled[i] != 0;
      }
      float w = 1.f;
      if (CONF) {                                                                   // numel = n_dep * W, W = (pooled sum of c) / 255
        const long long sc = conf_sum[b];
        w = (float)valid_pooled[i] / 255.f;
        gd = sc > 0 ? 50.f / (float)((double)d.n_dep * ((double)sc / 255.0)) * w : 0.f;
      }
      const float* tg = tgt_depth + ((long)(b * d.n_scales + s) * d.n_dep) * pp + pix;
      float* q = p + (long)d.n_sem * pp;
      const int c0 = ((int)blockIdx.y - 1) * DCH;
      // a depth-hot plane flagged "the constant 1" (live_planes == 1) was not pooled per room: its pooled plane is the same for every
      // room and lives in pooled_ones [n_scales][P][P] (built with the pooling kernel itself); its gradient, which nobody reads, is
      // not stored
      const float one_p = (live != nullptr && pooled_ones != nullptr) ? pooled_ones[(long)s * pp + pix] : 0.f;
      float a[DCH], t[DCH]; bool cst[DCH];
#pragma unroll
      for (int u = 0; u < DCH; ++u) {
        const int c = min(c0 + u, d.n_dep - 1);
        cst[u] = live != nullptr && pooled_ones != nullptr && live[b * d.C + d.dep0 + c] == 1;
        a[u] = cst[u] ? one_p : q[c * pp]; t[u] = ok ? tg[c * pp] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < DCH; ++u) {
        if (c0 + u < d.n_dep) {
          const float diff = a[u] - t[u];
          l_abs += ok ? (CONF ? w * fabsf(diff) : fabsf(diff)) : 0.f;
          if (!cst[u]) q[(c0 + u) * pp] = !ok ? 0.f : (diff > 0.f ? gd : (diff < 0.f ? -gd : 0.f));
        }
      }
    }
  }
  // block reduction; one partial per block (a same-address atomic per block is serialised on the memory side: with 1440
  // blocks the three atomics of the first version cost 60 us), summed in a fixed order by loss_finalize_kernel
  __shared__ float red[2][2];
  for (int o = 32; o > 0; o >>= 1) { l_abs += __shfl_down(l_abs, o, 64); l_ce += __shfl_down(l_ce, o, 64); }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = l_abs; red[wave][1] = l_ce; }
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = make_float2(red[0][0] + red[1][0], red[0][1] + red[1][1]);
}

// per_room: workgroup b sums room b's partials - gx blocks per part row of which the room owns bpr consecutive ones (a block of
// loss_kernel never straddles two rooms, checked by the launcher) - in the order the B = 1 launch sums its own
// depth_count (the masked route): the mean's element number is n_dep * depth_count[b] instead of the closed form; 0 gives depth 0
// conf_sum (the confidence route, with depth_count): n_dep * conf_sum[b] / 255, the partials being sums of w * |diff|
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float2* __restrict__ partial, int n, RefineDims d, float* __restrict__ loss_out,
                                                            const int gx, const int bpr, const int32_t* __restrict__ depth_count,
                                                            const int64_t* __restrict__ conf_sum) {
  __shared__ double red[4][2];
  double a = 0.0, c = 0.0;
  if (d.per_room) {
    const int b = blockIdx.x, ny = n / gx;
    loss_out += 3 * b;
    for (int i = threadIdx.x; i < ny * bpr; i += 256) { const float2 v = partial[(i / bpr) * gx + b * bpr + (i % bpr)]; a += (double)v.x; c += (double)v.y; }
  } else
  for (int i = threadIdx.x; i < n; i += 256) { const float2 v = partial[i]; a += (double)v.x; c += (double)v.y; }
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); c += __shfl_down(c, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0] + red[1][0] + red[2][0] + red[3][0]; c = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    double depth = 0.5 * a / ((double)(d.per_room ? 1 : d.B) * d.n_scales * d.n_dep * d.P * d.P);
    if (depth_count != nullptr) {
      const int nv = depth_count[d.per_room ? blockIdx.x : 0];
      depth = nv > 0 ? 0.5 * a / ((double)d.n_dep * nv) : 0.0;
    }
    if (conf_sum != nullptr) {                                                      // the confidence route: W = (pooled sum of c) / 255 in place of N
      const long long sc = conf_sum[d.per_room ? blockIdx.x : 0];
      depth = sc > 0 ? 0.5 * a / ((double)d.n_dep * ((double)sc / 255.0)) : 0.0;
    }
    loss_out[0] = (float)(100.0 * depth + 100.0 * c); loss_out[1] = (float)depth; loss_out[2] = (float)c;
  }
}

// The refinement report (testing/test_render_refine.py:369-374, what the reference pickles into bbox_rot_0.pkl): per room
//   depth_l1 = L1Loss(iter[:, 41:], target[:, 41:]) at full resolution, the iterate after the null fill (:332), the target as rendered
//   ce_last  = the cross-entropy of the last pooling scale, without the / 800
// report_depth_kernel: REPORT_BLOCKS workgroups per room, each over a run of pixels of all n_dep planes (dead planes enter as the
// constants they are, unread); report_finalize_kernel sums a room's partials and the last scale's blocks of loss_kernel's partials
// (a block of loss_kernel lies inside one (room, scale) when P * P is a multiple of 128) in a fixed order.
// MASKED (SlnRefineLoss::valid_image): a pixel outside the mask adds nothing and its target is not read; the mean's element number is
// n_dep * the room's valid pixels (depth_count row 1; 0 pixels: depth_l1 = 0).  Same loops, same order.
// MODE 2 (SlnRefineLoss::conf_sum): valid is the confidence image, a pixel with a byte c > 0 adds (c / 255.f) * |.| and the mean's
// element number is n_dep * (the room's image sum of c, conf_sum row 1) / 255.
constexpr int REPORT_BLOCKS = 64;
template <int MODE>
__global__ __launch_bounds__(256) void report_depth_kernel(const float* __restrict__ img, const float* __restrict__ tgt, const unsigned char* __restrict__ null,
                                                           const unsigned char* __restrict__ live, RefineDims d, double* __restrict__ scratch,
                                                           const unsigned char* __restrict__ valid) {
  constexpr bool MASKED = MODE != LOSS_PLAIN, CONF = MODE == LOSS_CONF;
  __shared__ double red[4];
  const int b = blockIdx.y;
  const long plane = (long)d.S * d.S, per = (plane + REPORT_BLOCKS - 1) / REPORT_BLOCKS;
  const long p0 = (long)blockIdx.x * per, p1 = p0 + per < plane ? p0 + per : plane;
  const float* src = img + ((long)b * d.C + d.dep0) * plane;
  const float* tg = tgt + (long)b * d.n_dep * plane;
  const unsigned char* nm = null + (long)b * plane;
  double acc = 0.0;
  for (int c = 0; c < d.n_dep; ++c) {
    const int lv = live != nullptr ? live[b * d.C + d.dep0 + c] : 3;
    const bool last = c == d.n_dep - 1;
    const float cst = (lv & 1) ? 1.f : 0.f;
    float a = 0.f;
    for (long p = p0 + threadIdx.x; p < p1; p += 256) {
      const int cf = MASKED ? valid[(long)b * plane + p] : 1;
      if (MASKED && !cf) continue;
      float v = lv == 3 ? src[c * plane + p] : cst;
      if (last && nm[p]) v = 1.f;
      a += CONF ? ((float)cf / 255.f) * fabsf(v - tg[c * plane + p]) : fabsf(v - tg[c * plane + p]);
    }
    acc += (double)a;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) scratch[b * REPORT_BLOCKS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void report_finalize_kernel(const double* __restrict__ scratch, const float2* __restrict__ partial, RefineDims d,
                                                             double* __restrict__ iou_mean, float* __restrict__ report,
                                                             const int32_t* __restrict__ image_count, const int64_t* __restrict__ image_sum) {
  const int b = blockIdx.x, bps = d.P * d.P / 128;                      // blocks of loss_kernel per (room, scale)
  double a = scratch[b * REPORT_BLOCKS + threadIdx.x], c = 0.0;
  const float2* ps = partial + (long)(b * d.n_scales + d.n_scales - 1) * bps;      // part row 0 (the semantic part), the last scale
  for (int i = threadIdx.x; i < bps; i += 64) c += (double)ps[i].y;
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); c += __shfl_down(c, o, 64); }
  if (threadIdx.x == 0) {
    float iou = __builtin_nanf("");
    if (iou_mean != nullptr) { iou = (float)iou_mean[b]; iou_mean[b] = 0.0; }
    report[3 * b + 0] = iou;
    double l1 = a / ((double)d.n_dep * d.S * d.S);
    if (image_count != nullptr) l1 = image_count[b] > 0 ? a / ((double)d.n_dep * image_count[b]) : 0.0;
    if (image_sum != nullptr) l1 = image_sum[b] > 0 ? a / ((double)d.n_dep * ((double)image_sum[b] / 255.0)) : 0.0;
    report[3 * b + 1] = (float)l1;
    report[3 * b + 2] = (float)(c * 800.0);
  }
}

// The validity mask of a target (sln_refine_loss_mask; once per target, in front of the loop).
//   refine_mask_kernel        one lane per pooled pixel, one workgroup inside one (room, scale): the AND over the 16 image pixels
//                             pool_kernel addresses for it - its index expressions, the weights ignored - is the pooled pixel's validity;
//                             an invalid one loses its label.  The taps are read as 16 single bytes: the mask of a room is S * S bytes (9 KB at
//                             96, 64 KB at 256) and stays in L1 / L2 for the 4 scales' lanes that read it, the two columns of a pair are
//                             adjacent only where i1 = i0 + 1 and sit on no 4-byte boundary, and the call runs once per target - staging
//                             the intermediate through LDS as pool_lds_kernel does would buy nothing here.
//   refine_mask_image_kernel  the non-zero pixels of a room's mask (the report's element number)
//   counts: a ballot per wavefront, one integer atomic per workgroup and counter - exact, the same in any order - into counters
//   that a launch of their own clears; refine_mask_finalize_kernel turns them into inv_count, depth_count and mask_status.
//   cnt layout (int32, in the loss workspace): [B][n_scales] labels kept, [B][n_scales] valid pooled pixels, [B] valid image pixels
__global__ void refine_mask_clear_kernel(int* __restrict__ cnt, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cnt[i] = 0;
}

__global__ __launch_bounds__(256) void refine_mask_kernel(const unsigned char* __restrict__ valid, RefineDims d,
                                                          const int* __restrict__ s2_k0, const int* __restrict__ s2_k1,
                                                          const int* __restrict__ s1_i0, const int* __restrict__ s1_i1,
                                                          int* __restrict__ labels, unsigned char* __restrict__ valid_pooled, int* __restrict__ cnt) {
  const int pp = d.P * d.P;
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int s = blockIdx.y % d.n_scales, b = blockIdx.y / d.n_scales;
  bool ok = false, lab = false;
  if (o < pp) {
    const int oy = o / d.P, ox = o % d.P;
    const int ky[2] = {s2_k0[s * d.P + oy], s2_k1[s * d.P + oy]}, kx[2] = {s2_k0[s * d.P + ox], s2_k1[s * d.P + ox]};
    int yy[4], xx[4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      yy[2 * a] = s1_i0[s * d.pmax + ky[a]]; yy[2 * a + 1] = s1_i1[s * d.pmax + ky[a]];
      xx[2 * a] = s1_i0[s * d.pmax + kx[a]]; xx[2 * a + 1] = s1_i1[s * d.pmax + kx[a]];
    }
    const unsigned char* vm = valid + (long)b * d.S * d.S;
    ok = true;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) ok = ok && vm[(long)yy[a] * d.S + xx[e]] != 0;
    const long i = ((long)b * d.n_scales + s) * pp + o;
    valid_pooled[i] = ok ? 1 : 0;
    if (!ok) labels[i] = -100;
    lab = ok && labels[i] >= 0;
  }
  __shared__ int red[4][2];
  const int c_ok = __popcll(__ballot(ok)), c_lab = __popcll(__ballot(lab));
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = c_lab; red[threadIdx.x >> 6][1] = c_ok; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n_lab = red[0][0] + red[1][0] + red[2][0] + red[3][0], n_ok = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    if (n_lab) atomicAdd(cnt + b * d.n_scales + s, n_lab);                       // (integers: the total does not depend on the order)
    if (n_ok) atomicAdd(cnt + (d.B + b) * d.n_scales + s, n_ok);
  }
}

__global__ __launch_bounds__(256) void refine_mask_image_kernel(const unsigned char* __restrict__ valid, RefineDims d, int* __restrict__ cnt) {
  const int plane = d.S * d.S, p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  const bool ok = p < plane && valid[(long)b * plane + p] != 0;
  __shared__ int red[4];
  const int c = __popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = red[0] + red[1] + red[2] + red[3];
    if (n) atomicAdd(cnt + 2 * d.B * d.n_scales + b, n);
  }
}

// one workgroup, a thread per room (strided): B * n_scales is a few dozen numbers
__global__ __launch_bounds__(256) void refine_mask_finalize_kernel(const int* __restrict__ cnt, RefineDims d, float* __restrict__ inv_count,
                                                                   int* __restrict__ depth_count, int* __restrict__ mask_status) {
  const int ns = d.n_scales;
  const int* c_lab = cnt; const int* c_ok = cnt + d.B * ns; const int* c_img = cnt + 2 * d.B * ns;
  for (int b = threadIdx.x; b < d.B; b += 256) {
    int n = 0, none = 0;
    if (d.per_room) {
      for (int s = 0; s < ns; ++s) { n += c_ok[b * ns + s]; none |= c_lab[b * ns + s] == 0; inv_count[b * ns + s] = 1.f / (float)c_lab[b * ns + s]; }
    } else {
      for (int s = 0; s < ns; ++s) {
        int l = 0;
        for (int r = 0; r < d.B; ++r) { n += c_ok[r * ns + s]; l += c_lab[r * ns + s]; }
        none |= l == 0;
        if (b == 0) inv_count[s] = 1.f / (float)l;
      }
    }
    depth_count[b] = n; depth_count[d.B + b] = c_img[b];
    mask_status[b] = (n == 0 ? 1 : 0) | (none ? 2 : 0);
  }
}

// The per-pixel confidence of a target (sln_refine_loss_confidence; once per target, the launch structure of the mask call).
//   refine_conf_kernel        refine_mask_kernel with the MINIMUM over the 16 taps in place of the AND: the pooled confidence byte; a
//                             pooled pixel with byte 0 loses its label
//   refine_conf_image_kernel  the non-zero pixels and the sum of a room's confidence image (the report's normalisers)
//   sums: the lanes' bytes are added per wavefront (64 * 255 fits an int), the four wavefronts through LDS, then one 64-bit integer
//   atomic per workgroup and counter (an image's sum of bytes passes 2^31 from S = 4096) - exact, the same in any order.
//   cnt layout (64-bit, at the head of the pooled maps): [B][n_scales] sum of c over the kept labels, [B][n_scales] pooled pixels with
//   c > 0, [B][n_scales] sum of c over the pooled pixels, [B] image pixels with c > 0, [B] sum of c over the image
typedef unsigned long long conf_cnt_t;
__global__ void refine_conf_clear_kernel(conf_cnt_t* __restrict__ cnt, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cnt[i] = 0;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void refine_conf_kernel(const unsigned char* __restrict__ conf, RefineDims d,
                                                          const int* __restrict__ s2_k0, const int* __restrict__ s2_k1,
                                                          const int* __restrict__ s1_i0, const int* __restrict__ s1_i1,
                                                          int* __restrict__ labels, unsigned char* __restrict__ conf_pooled,
                                                          conf_cnt_t* __restrict__ cnt) {
  const int pp = d.P * d.P;
  const int o = blockIdx.x * 256 + threadIdx.x;
  const int s = blockIdx.y % d.n_scales, b = blockIdx.y / d.n_scales;
  int c = 0, c_lab = 0;
  if (o < pp) {
    const int oy = o / d.P, ox = o % d.P;
    const int ky[2] = {s2_k0[s * d.P + oy], s2_k1[s * d.P + oy]}, kx[2] = {s2_k0[s * d.P + ox], s2_k1[s * d.P + ox]};
    int yy[4], xx[4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      yy[2 * a] = s1_i0[s * d.pmax + ky[a]]; yy[2 * a + 1] = s1_i1[s * d.pmax + ky[a]];
      xx[2 * a] = s1_i0[s * d.pmax + kx[a]]; xx[2 * a + 1] = s1_i1[s * d.pmax + kx[a]];
    }
    const unsigned char* cm = conf + (long)b * d.S * d.S;
    c = 255;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) c = min(c, (int)cm[(long)yy[a] * d.S + xx[e]]);
    const long i = ((long)b * d.n_scales + s) * pp + o;
    conf_pooled[i] = (unsigned char)c;
    if (c == 0) labels[i] = -100;
    c_lab = (c != 0 && labels[i] >= 0) ? c : 0;
  }
  __shared__ int red[4][3];
  const int w_lab = wave_sum(c_lab), w_ok = __popcll(__ballot(c != 0)), w_c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = w_lab; red[threadIdx.x >> 6][1] = w_ok; red[threadIdx.x >> 6][2] = w_c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n_lab = red[0][0] + red[1][0] + red[2][0] + red[3][0], n_ok = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    const int n_c = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    const int bs = b * d.n_scales + s, nbs = d.B * d.n_scales;
    if (n_lab) atomicAdd(cnt + bs, (conf_cnt_t)n_lab);                             // (integers: the total does not depend on the order)
    if (n_ok) { atomicAdd(cnt + nbs + bs, (conf_cnt_t)n_ok); atomicAdd(cnt + 2 * nbs + bs, (conf_cnt_t)n_c); }
  }
}

__global__ __launch_bounds__(256) void refine_conf_image_kernel(const unsigned char* __restrict__ conf, RefineDims d, conf_cnt_t* __restrict__ cnt) {
  const long plane = (long)d.S * d.S, p = (long)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  const int c = p < plane ? conf[(long)b * plane + p] : 0;
  __shared__ int red[4][2];
  const int w_ok = __popcll(__ballot(c != 0)), w_c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = w_ok; red[threadIdx.x >> 6][1] = w_c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = red[0][0] + red[1][0] + red[2][0] + red[3][0], n_c = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    conf_cnt_t* img = cnt + 3 * d.B * d.n_scales;
    if (n) { atomicAdd(img + b, (conf_cnt_t)n); atomicAdd(img + d.B + b, (conf_cnt_t)n_c); }
  }
}

// one workgroup, a thread per room (strided)
__global__ __launch_bounds__(256) void refine_conf_finalize_kernel(const conf_cnt_t* __restrict__ cnt, RefineDims d, float* __restrict__ inv_count,
                                                                   int* __restrict__ depth_count, int64_t* __restrict__ conf_sum,
                                                                   int* __restrict__ mask_status) {
  const int ns = d.n_scales;
  const conf_cnt_t* c_lab = cnt; const conf_cnt_t* c_ok = cnt + d.B * ns; const conf_cnt_t* c_sum = cnt + 2 * d.B * ns;
  const conf_cnt_t* c_img = cnt + 3 * d.B * ns;
  for (int b = threadIdx.x; b < d.B; b += 256) {
    conf_cnt_t n = 0, sc = 0;
    int none = 0;
    if (d.per_room) {
      for (int s = 0; s < ns; ++s) {
        n += c_ok[b * ns + s]; sc += c_sum[b * ns + s]; none |= c_lab[b * ns + s] == 0;
        inv_count[b * ns + s] = 1.f / (float)((double)c_lab[b * ns + s] / 255.0);
      }
    } else {
      for (int s = 0; s < ns; ++s) {
        conf_cnt_t l = 0;
        for (int r = 0; r < d.B; ++r) { n += c_ok[r * ns + s]; sc += c_sum[r * ns + s]; l += c_lab[r * ns + s]; }
        none |= l == 0;
        if (b == 0) inv_count[s] = 1.f / (float)((double)l / 255.0);
      }
    }
    depth_count[b] = (int)n; depth_count[d.B + b] = (int)c_img[b];
    conf_sum[b] = (int64_t)sc; conf_sum[d.B + b] = (int64_t)c_img[d.B + b];
    mask_status[b] = (n == 0 ? 1 : 0) | (none ? 2 : 0);
  }
}

// d loss / d image[b][c][y][x] = gscale * sum_s sum_{(oy, wy) in col_s(y)} sum_{(ox, wx) in col_s(x)} wy wx dpooled[b][s][c][oy][ox]
__global__ __launch_bounds__(256) void refine_bwd_kernel(const float* __restrict__ dpooled, const unsigned char* __restrict__ null, RefineDims d,
                                                         const int* __restrict__ col_ptr, const int* __restrict__ col_out,
                                                         const float* __restrict__ col_w, const float* __restrict__ gscale,
                                                         float* __restrict__ dimg) {
  const long plane = (long)d.S * d.S;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)d.B * d.C * plane) return;
  const int x = (int)(i % d.S), y = (int)((i / d.S) % d.S);
  const int c = (int)((i / plane) % d.C), b = (int)(i / (plane * d.C));
  const int nc = d.n_sem + d.n_dep, cc = c - d.sem0;
  float g = 0.f;
  if (cc >= 0 && cc < nc && !(c == d.dep0 + d.n_dep - 1 && null[(long)b * plane + (long)y * d.S + x])) {
    const long pp = (long)d.P * d.P;
    for (int s = 0; s < d.n_scales; ++s) {
      const int* cp = col_ptr + s * (d.S + 1);
      const int yb = cp[y], ye = cp[y + 1], xb = cp[x], xe = cp[x + 1];
      if (yb == ye || xb == xe) continue;
      const float* dp = dpooled + ((long)(b * d.n_scales + s) * nc + cc) * pp;
      for (int e = yb; e < ye; ++e) {
        const float wy = col_w[e];
        const float* row = dp + (long)col_out[e] * d.P;
        float r = 0.f;
        for (int f = xb; f < xe; ++f) r = fmaf(col_w[f], row[col_out[f]], r);
        g = fmaf(wy, r, g);
      }
    }
    g *= gscale[0];
  }
  dimg[i] = g;
}

// The same sum, separable, with one workgroup per (strip of ROWS image rows, channel):
//   stage 1  T[s][r][ox] = sum_{(oy, wy) in col_s(y0 + r)} wy * dpooled[s][c][oy][ox]      rows of dpooled, coalesced, into LDS
//   stage 2  g[r][x]     = sum_s sum_{(ox, wx) in col_s(x)} wx * T[s][r][ox]                 LDS reads only
// A lane owns one image column and keeps that column's tap lists (padded to MAXX entries per scale, weight 0) in registers
// for all rows of the strip.  The generic kernel above walks four CSR ranges per (pixel, channel) through dependent global
// loads (136 us per 256 x 256 x 70 gradient; 61 us with its inner loop padded, L1-issue bound); this one takes 41 us.
template <int MAXX, int ROWS, int PMAX>
__global__ __launch_bounds__(256) void refine_bwd_sep_kernel(const float* __restrict__ dpooled, const unsigned char* __restrict__ null,
                                                             RefineDims d, const int* __restrict__ col_ptr, const int* __restrict__ col_out,
                                                             const float* __restrict__ col_w, const float* __restrict__ gscale,
                                                             float* __restrict__ dimg, const unsigned char* __restrict__ live) {
  __shared__ float T[MAX_SCALES][ROWS][PMAX];
  const int x = blockIdx.z * 256 + threadIdx.x;
  const int c = blockIdx.y % d.C, b = blockIdx.y / d.C;
  const int y0 = blockIdx.x * ROWS;
  const bool active = x < d.S;
  const int xs = active ? x : d.S - 1;
  const int nc = d.n_sem + d.n_dep, cc = c - d.sem0;
  float* out = dimg + ((long)(b * d.C + c) * d.S) * d.S;
  if (live != nullptr && cc >= 0 && cc < nc && !(live[b * d.C + c] & 2)) return;      // a plane nobody reads the gradient of (live_planes): left as it is
  if (cc < 0 || cc >= nc) {                                                            // channel 0
    if (active) for (int r = 0; r < ROWS && y0 + r < d.S; ++r) out[(long)(y0 + r) * d.S + x] = 0.f;
    return;
  }
  int ox[MAX_SCALES][MAXX]; float wx[MAX_SCALES][MAXX];
#pragma unroll
  for (int s = 0; s < MAX_SCALES; ++s) {
    const int sv = s < d.n_scales ? s : 0;
    const int xb = col_ptr[sv * (d.S + 1) + xs], xe = s < d.n_scales ? col_ptr[sv * (d.S + 1) + xs + 1] : xb;
#pragma unroll
    for (int f = 0; f < MAXX; ++f) {
      const bool v = xb + f < xe;
      ox[s][f] = v ? col_out[xb + f] : 0;
      wx[s][f] = v ? col_w[xb + f] : 0.f;
    }
  }
  // the strip's row lists, padded like the column lists, so that stage 1 issues MAXX independent loads per element
  __shared__ int yo[MAX_SCALES * ROWS][MAXX];
  __shared__ float yw[MAX_SCALES * ROWS][MAXX];
  for (int i = threadIdx.x; i < d.n_scales * ROWS * MAXX; i += 256) {
    const int e = i % MAXX, r = (i / MAXX) % ROWS, s = i / (MAXX * ROWS);
    const int y = min(y0 + r, d.S - 1);
    const int yb = col_ptr[s * (d.S + 1) + y], ye = col_ptr[s * (d.S + 1) + y + 1];
    const bool v = yb + e < ye && y0 + r < d.S;
    yo[s * ROWS + r][e] = v ? col_out[yb + e] : 0;
    yw[s * ROWS + r][e] = v ? col_w[yb + e] : 0.f;
  }
  __syncthreads();
  const long pp = (long)d.P * d.P;
  // four elements per pass, their 4 x MAXX loads issued together: one element at a time (MAXX loads in flight per thread, 24 dependent
  // round trips per workgroup) left the kernel latency-bound - 405 us for 16 rooms against ~130 us of LDS + L1 issue time
  {
    const int n1 = d.n_scales * ROWS * d.P;
    constexpr int U = 4;
    for (int i0 = threadIdx.x; i0 < n1; i0 += 256 * U) {
      float v[U][MAXX]; float wgt[U][MAXX]; int si[U], ri[U], oi[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = min(i0 + 256 * u, n1 - 1);
        oi[u] = i % d.P; ri[u] = (i / d.P) % ROWS; si[u] = i / (d.P * ROWS);
        const float* dp = dpooled + ((long)(b * d.n_scales + si[u]) * nc + cc) * pp + oi[u];
#pragma unroll
        for (int e = 0; e < MAXX; ++e) { wgt[u][e] = yw[si[u] * ROWS + ri[u]][e]; v[u][e] = dp[(long)yo[si[u] * ROWS + ri[u]][e] * d.P]; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (i0 + 256 * u < n1) {
          float t = 0.f;
#pragma unroll
          for (int e = 0; e < MAXX; ++e) t = fmaf(wgt[u][e], v[u][e], t);
          T[si[u]][ri[u]][oi[u]] = t;
        }
      }
    }
  }
  __syncthreads();
  if (!active) return;
  const float gs = gscale[0];
  const bool last = c == d.dep0 + d.n_dep - 1;
  for (int r = 0; r < ROWS && y0 + r < d.S; ++r) {
    float g = 0.f;
    // (a scale the descriptor does not have has no row of T: stage 1 never wrote it, and a weight of 0 does not make what LDS holds
    //  there harmless - 0 * NaN is NaN)
#pragma unroll
    for (int s = 0; s < MAX_SCALES; ++s)
      if (s < d.n_scales)
#pragma unroll
        for (int f = 0; f < MAXX; ++f) g = fmaf(wx[s][f], T[s][r][ox[s][f]], g);
    if (last && null[(long)b * d.S * d.S + (long)(y0 + r) * d.S + x]) g = 0.f;
    out[(long)(y0 + r) * d.S + x] = g * gs;
  }
}

}  // namespace

extern "C" {

int64_t sln_refine_loss_workspace_bytes(int B, int image_size, int pooled_size, int n_scales, int n_sem, int n_dep) {
  if (B <= 0 || image_size <= 0 || pooled_size <= 0 || n_scales <= 0 || n_scales > MAX_SCALES || n_sem <= 0 || n_dep <= 0) return SLN_E_BADARG;
  const int64_t pooled = (int64_t)B * n_scales * (n_sem + n_dep) * pooled_size * pooled_size * 4;
  const int64_t mask = ((int64_t)B * image_size * image_size + 255) / 256 * 256;
  const int64_t nblk = (((int64_t)B * n_scales * pooled_size * pooled_size + 127) / 128) * (1 + (n_dep + DCH - 1) / DCH);
  return pooled + mask + nblk * 8;                    // + one float2 partial per block of loss_kernel
}

static int carve(const SlnRefineLoss* L, void* workspace, float** pooled, unsigned char** mask, float2** partial) {
  char* p = (char*)workspace;
  const int64_t np = (int64_t)L->B * L->n_scales * (L->n_sem + L->n_dep) * L->pooled_size * L->pooled_size * 4;
  const int64_t nm = ((int64_t)L->B * L->image_size * L->image_size + 255) / 256 * 256;
  *pooled = (float*)p; *mask = (unsigned char*)(p + np); *partial = (float2*)(p + np + nm);
  return 0;
}

static int check(const SlnRefineLoss* L) {
  if (!L || L->B <= 0 || L->image_size <= 0 || L->pooled_size <= 0 || L->n_scales <= 0 || L->n_scales > MAX_SCALES) return SLN_E_BADARG;
  if (L->n_sem != 40) return SLN_E_UNSUPPORTED;      // NYU-40 one-hot block of the scene tensor (models/diff_render.py:3)
  if (L->sem0 < 0 || L->dep0 != L->sem0 + L->n_sem || L->dep0 + L->n_dep > L->channels || L->n_dep <= 0) return SLN_E_BADARG;
  if (!L->s2_k0 || !L->s2_k1 || !L->s2_l1 || !L->s1_i0 || !L->s1_i1 || !L->s1_l1 || !L->col_ptr || !L->col_out || !L->col_w) return SLN_E_BADARG;
  // per_room: a 128-row block of loss_kernel must not cover two rooms (checked here - init and every entry point - so that an
  // unsupported geometry fails before anything is launched or overwritten)
  if (L->per_room && ((long)L->n_scales * L->pooled_size * L->pooled_size) % 128 != 0) return SLN_E_UNSUPPORTED;
  // the validity mask: all three fields or none
  const int n_mask = (L->valid_pooled != nullptr) + (L->valid_image != nullptr) + (L->depth_count != nullptr);
  if (n_mask != 0 && n_mask != 3) return SLN_E_BADARG;
  // the confidence sums reinterpret the three mask fields: never without them
  if (L->conf_sum != nullptr && n_mask != 3) return SLN_E_BADARG;
  return 0;
}

static RefineDims dims_of(const SlnRefineLoss* L) {
  RefineDims d;
  d.B = L->B; d.S = L->image_size; d.P = L->pooled_size; d.C = L->channels; d.sem0 = L->sem0; d.n_sem = L->n_sem; d.dep0 = L->dep0;
  d.n_dep = L->n_dep; d.n_scales = L->n_scales; d.pmax = L->stage1_stride;
  d.per_room = L->per_room != 0; d.pad_ = 0;
  return d;
}

int sln_refine_loss_init(const SlnRefineLoss* L, void* workspace, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!workspace) return SLN_E_BADARG;
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, workspace, &pooled, &mask, &partial);
  (void)pooled; (void)mask; (void)partial; (void)stream;       // nothing to arm: every call rewrites what it reads
  return 0;
}

// live_planes is honoured only where every kernel of the forward / backward pair knows about it (the LDS pooling kernel and the
// separable backward kernel: the shapes of the refinement loop); elsewhere every plane is processed
static const unsigned char* live_of(const SlnRefineLoss* L, const RefineDims& d) {
  const bool ok = d.pmax <= POOL_LDS_MAX && d.P <= POOL_LDS_MAX && L->max_col_entries > 0 && L->max_col_entries <= 5 && d.n_sem == 40;
  return ok ? L->live_planes : nullptr;
}

static void launch_pool(const SlnRefineLoss* L, const RefineDims& d, const float* image, int null_fill, unsigned char* mask, float* pooled,
                        const unsigned char* live, hipStream_t st) {
  const long npix = (long)d.B * d.S * d.S;
  if (null_fill == 1) hipLaunchKernelGGL(null_mask_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, image, d, mask, live);      // 2: `mask` is given
  if (d.pmax <= POOL_LDS_MAX && d.P <= POOL_LDS_MAX) {
    hipLaunchKernelGGL(pool_lds_kernel, dim3(d.B * (d.n_sem + d.n_dep), d.n_scales), dim3(256), 0, st, image, mask, null_fill, d, L->s2_k0, L->s2_k1,
                       L->s2_l1, L->s1_i0, L->s1_i1, L->s1_l1, pooled, live, (live != nullptr && L->pooled_ones != nullptr) ? 1 : 0);
    return;
  }
  const long np = (long)d.B * d.n_scales * sln_cdiv(d.n_sem + d.n_dep, CG) * d.P * d.P;
  hipLaunchKernelGGL(pool_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, image, mask, null_fill, d, L->s2_k0, L->s2_k1, L->s2_l1,
                     L->s1_i0, L->s1_i1, L->s1_l1, pooled);
}

int sln_refine_pool(const SlnRefineLoss* L, const float* image, int null_fill, void* workspace, float* pooled_out, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!image || !workspace || !pooled_out) return SLN_E_BADARG;
  const RefineDims d = dims_of(L);
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, workspace, &pooled, &mask, &partial);
  launch_pool(L, d, image, null_fill, mask, pooled_out, nullptr, (hipStream_t)stream);      // any image: no plane is known dead
  SLN_CHECK_LAUNCH();
  return 0;
}

// 1 when live_planes (and with it null_mask / pooled_ones) of this descriptor would be honoured - the shapes the LDS pooling kernel
// and the separable backward kernel take; 0 when every plane is processed regardless.  A producer that leaves dead planes of the
// image unwritten (sln_scene_forward_live) must not be paired with a loss that reads them: ask first.
int sln_refine_loss_live_ok(const SlnRefineLoss* L) {
  if (check(L)) return 0;
  SlnRefineLoss probe = *L;
  static const unsigned char one = 1;
  probe.live_planes = &one;                       // (only compared against NULL)
  return live_of(&probe, dims_of(&probe)) != nullptr ? 1 : 0;
}

int sln_refine_loss_forward(const SlnRefineLoss* L, const float* image, const float* target_depth_pooled, const int32_t* labels,
                            const float* inv_count, void* workspace, float* loss_out, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!image || !target_depth_pooled || !labels || !inv_count || !workspace || !loss_out) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const RefineDims d = dims_of(L);
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, workspace, &pooled, &mask, &partial);
  const unsigned char* live = live_of(L, d);
  // the null mask as the producer of `image` computed it (SlnRefineLoss::null_mask: the scene pass's compose kernel sums the 29
  // depth-hot values of a pixel in this kernel's order while it has them in registers): null_mask_kernel's launch is skipped
  const bool ext_mask = live != nullptr && L->null_mask != nullptr;
  if (ext_mask) mask = const_cast<unsigned char*>(L->null_mask);
  launch_pool(L, d, image, ext_mask ? 2 : 1, mask, pooled, live, st);
  const long nl = (long)d.B * d.n_scales * d.P * d.P;
  const dim3 lg((unsigned)((nl + 127) / 128), 1 + sln_cdiv(d.n_dep, DCH));
  if (L->conf_sum != nullptr)
    hipLaunchKernelGGL((loss_kernel<40, LOSS_CONF>), lg, dim3(128), 0, st, pooled, d, target_depth_pooled, labels, inv_count, partial, live,
                       L->pooled_ones, L->valid_pooled, L->depth_count, L->conf_sum);
  else if (L->valid_pooled != nullptr)
    hipLaunchKernelGGL((loss_kernel<40, LOSS_MASKED>), lg, dim3(128), 0, st, pooled, d, target_depth_pooled, labels, inv_count, partial, live,
                       L->pooled_ones, L->valid_pooled, L->depth_count, (const int64_t*)nullptr);
  else
    hipLaunchKernelGGL((loss_kernel<40, LOSS_PLAIN>), lg, dim3(128), 0, st, pooled, d, target_depth_pooled, labels, inv_count, partial, live,
                       L->pooled_ones, (const unsigned char*)nullptr, (const int32_t*)nullptr, (const int64_t*)nullptr);
  const long per_room_rows = (long)d.n_scales * d.P * d.P;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(d.per_room ? d.B : 1), dim3(256), 0, st, partial, (int)(lg.x * lg.y), d, loss_out, (int)lg.x,
                     (int)(per_room_rows / 128), L->valid_pooled != nullptr ? L->depth_count : (const int32_t*)nullptr, L->conf_sum);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_refine_loss_mask(const SlnRefineLoss* L, const unsigned char* valid, int32_t* labels, unsigned char* valid_pooled, float* inv_count,
                         int32_t* depth_count, int32_t* mask_status, void* workspace, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!valid || !labels || !valid_pooled || !inv_count || !depth_count || !mask_status || !workspace) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const RefineDims d = dims_of(L);
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, workspace, &pooled, &mask, &partial);
  int* cnt = reinterpret_cast<int*>(pooled);                  // (2 n_scales + 1) B counters at the head of the pooled maps, which every forward rewrites
  const int n_cnt = (2 * d.n_scales + 1) * d.B;
  hipLaunchKernelGGL(refine_mask_clear_kernel, dim3(sln_cdiv(n_cnt, 256)), dim3(256), 0, st, cnt, n_cnt);
  hipLaunchKernelGGL(refine_mask_kernel, dim3(sln_cdiv(d.P * d.P, 256), d.B * d.n_scales), dim3(256), 0, st, valid, d, L->s2_k0, L->s2_k1, L->s1_i0,
                     L->s1_i1, labels, valid_pooled, cnt);
  hipLaunchKernelGGL(refine_mask_image_kernel, dim3(sln_cdiv(d.S * d.S, 256), d.B), dim3(256), 0, st, valid, d, cnt);
  hipLaunchKernelGGL(refine_mask_finalize_kernel, dim3(1), dim3(256), 0, st, cnt, d, inv_count, depth_count, mask_status);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_refine_loss_confidence(const SlnRefineLoss* L, const unsigned char* conf, int32_t* labels, unsigned char* conf_pooled, float* inv_count,
                               int32_t* depth_count, int64_t* conf_sum, int32_t* mask_status, void* workspace, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!conf || !labels || !conf_pooled || !inv_count || !depth_count || !conf_sum || !mask_status || !workspace) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const RefineDims d = dims_of(L);
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, workspace, &pooled, &mask, &partial);
  conf_cnt_t* cnt = reinterpret_cast<conf_cnt_t*>(pooled);    // (3 n_scales + 2) B 64-bit counters at the head of the pooled maps, which every forward rewrites
  const int n_cnt = (3 * d.n_scales + 2) * d.B;
  hipLaunchKernelGGL(refine_conf_clear_kernel, dim3(sln_cdiv(n_cnt, 256)), dim3(256), 0, st, cnt, n_cnt);
  hipLaunchKernelGGL(refine_conf_kernel, dim3(sln_cdiv(d.P * d.P, 256), d.B * d.n_scales), dim3(256), 0, st, conf, d, L->s2_k0, L->s2_k1, L->s1_i0,
                     L->s1_i1, labels, conf_pooled, cnt);
  hipLaunchKernelGGL(refine_conf_image_kernel, dim3((unsigned)(((long)d.S * d.S + 255) / 256), d.B), dim3(256), 0, st, conf, d, cnt);
  hipLaunchKernelGGL(refine_conf_finalize_kernel, dim3(1), dim3(256), 0, st, cnt, d, inv_count, depth_count, conf_sum, mask_status);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_refine_loss_backward(const SlnRefineLoss* L, const void* workspace, const float* grad_scale, float* grad_image, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!workspace || !grad_scale || !grad_image) return SLN_E_BADARG;
  const RefineDims d = dims_of(L);
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, const_cast<void*>(workspace), &pooled, &mask, &partial);
  const unsigned char* live = live_of(L, d);
  if (live != nullptr && L->null_mask != nullptr) mask = const_cast<unsigned char*>(L->null_mask);
  if (L->max_col_entries > 0 && L->max_col_entries <= 5 && d.P <= 96) {
    constexpr int ROWS = 16;
    hipLaunchKernelGGL((refine_bwd_sep_kernel<5, ROWS, 96>), dim3(sln_cdiv(d.S, ROWS), d.B * d.C, sln_cdiv(d.S, 256)), dim3(256), 0,
                       (hipStream_t)stream, pooled, mask, d, L->col_ptr, L->col_out, L->col_w, grad_scale, grad_image, live);
  } else {
    const long n = (long)d.B * d.C * d.S * d.S;
    hipLaunchKernelGGL(refine_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pooled, mask, d, L->col_ptr,
                       L->col_out, L->col_w, grad_scale, grad_image);
  }
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_refine_report(const SlnRefineLoss* L, const float* image, const float* target_depth, const void* workspace, double* scratch,
                      double* iou_mean, float* report_out, void* stream) {
  int r = check(L);
  if (r) return r;
  if (!image || !target_depth || !workspace || !scratch || !report_out) return SLN_E_BADARG;
  const RefineDims d = dims_of(L);
  if ((d.P * d.P) % 128 != 0 || (!d.per_room && d.B != 1)) return SLN_E_UNSUPPORTED;
  float* pooled; unsigned char* mask; float2* partial;
  carve(L, const_cast<void*>(workspace), &pooled, &mask, &partial);
  const unsigned char* live = live_of(L, d);
  if (live != nullptr && L->null_mask != nullptr) mask = const_cast<unsigned char*>(L->null_mask);
  hipStream_t st = (hipStream_t)stream;
  if (L->conf_sum != nullptr)
    hipLaunchKernelGGL(report_depth_kernel<LOSS_CONF>, dim3(REPORT_BLOCKS, d.B), dim3(256), 0, st, image, target_depth, mask, live, d, scratch, L->valid_image);
  else if (L->valid_image != nullptr)
    hipLaunchKernelGGL(report_depth_kernel<LOSS_MASKED>, dim3(REPORT_BLOCKS, d.B), dim3(256), 0, st, image, target_depth, mask, live, d, scratch, L->valid_image);
  else
    hipLaunchKernelGGL(report_depth_kernel<LOSS_PLAIN>, dim3(REPORT_BLOCKS, d.B), dim3(256), 0, st, image, target_depth, mask, live, d, scratch,
                       (const unsigned char*)nullptr);
  hipLaunchKernelGGL(report_finalize_kernel, dim3(d.B), dim3(64), 0, st, scratch, partial, d, iou_mean, report_out,
                     L->valid_image != nullptr ? L->depth_count + d.B : (const int32_t*)nullptr,
                     L->conf_sum != nullptr ? L->conf_sum + d.B : (const int64_t*)nullptr);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_refine_report_scratch_doubles(int B) { return B > 0 ? B * REPORT_BLOCKS : 0; }

}  // extern "C"
