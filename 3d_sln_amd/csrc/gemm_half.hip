// fp16-MFMA forms of the NT product for the VAE's eval-mode Linears (opt-in precision modes "f16" and "f16x3", DESIGN §4 A-half).
//
//   Y[:, ycol0 .. ycol0 + N) = op(A)[M, K] * W[N, K]^T (+ bias)      on v_mfma_f32_32x32x16_f16
//
// op(A) is the family's Operand (up to three row-gathered segments, per-column max(c0 x + c2, floor) from sln_coef_for) and W the
// fp32 parameter itself: BOTH are split into fp16 parts while they are staged, the scheme of conv_f16_kernel (spade.hip):
//   hi = (half)clamp(v, +-65504) (NaN kept), lo = (half)(clamp(v) - (float)hi)
//   terms = 1: y = sum a_hi w_hi                                      ("f16": operands rounded to 11 bits)
//   terms = 3: y = sum a_hi w_lo + a_lo w_hi + a_hi w_hi, in that order per 16-k step ("f16x3": fp16 products are exact in fp32 and the
//              dropped a_lo w_lo is 2^-22 of a product, so the result is fp32-grade)
// No packed copy of the weights is kept (parameters change under the optimizers, load_state_dict and params_changed()).
//
// Tiles: 128 rows x 128 or 64 columns per workgroup of 256 threads, wavefronts 2 x 2, each 64 x 64 or 64 x 32 of 32 x 32 MFMA blocks;
// whole 32-column blocks behind N are skipped.  K is walked in chunks of 32 = two MFMA steps of 16; the last chunk of a K that is
// 16 (mod 32) runs one step.  Staging goes through registers (global_load_lds cannot convert): the loads of chunk kt + 1 are issued
// in front of the MFMAs of chunk kt, converted and written to the one LDS buffer behind them (two barriers per chunk; two to three
// workgroups share a CU and run under each other's barriers).
//
// LDS layout: per part (hi, lo) [rows][40] halves - 32 k-contiguous halves and 8 of padding, a row stride of 80 bytes = 5 16-byte
// slots.  Lane l of a fragment read takes the 8 consecutive k of step s at row (l & 31), k = 16 s + 8 (l >> 5): ONE ds_read_b128.
// A ds_read_b128 is serviced in four groups of 16 lanes, each inside one 32-lane half (same k slot) and covering 16 rows that are
// distinct modulo 16 ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}); with an odd slot stride (5) 16 such rows fall on the 16
// different slots of the 256-byte bank row: conflict-free.  A staging thread writes the 8 halves of its granule as one 16-byte store.
//
// Every output element is ONE chain of MFMAs in fixed k order (no split-K, no atomics): a row's bits depend neither on M nor on
// where the row sits in the launch.
#include <cstdio>
#include <cstdlib>
#include "gemm_bodies.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int HBM = 128;          // rows per workgroup
constexpr int HBK = 32;           // k per staged chunk
constexpr int HLD = HBK + 8;      // LDS row stride in halves (see above)
constexpr int HK_MAX = 4096;      // the coefficient table of a wider operand would not fit the LDS next to the tiles

// one granule (8 consecutive k of one row) -> its fp16 parts
template <int TERMS>
__device__ __forceinline__ void half_split8(const float4 u, const float4 w, f16x8& hi, f16x8& lo) {
  const float x[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = x[k] != x[k] ? x[k] : fminf(fmaxf(x[k], -65504.f), 65504.f);      // NaN stays NaN (fmaxf would drop it)
    const _Float16 h = (_Float16)v;
    hi[k] = h;
    if (TERMS == 3) lo[k] = (_Float16)(v - (float)h);
  }
}

// TNB: 32-column blocks per wavefront (workgroup tile 128 x 64 TNB); IDENT: no coefficient table; MULTI: more than one segment
// (the segment is chosen per staging thread from its granule's column: boundaries are multiples of 16, a granule never straddles)
template <int TNB, int TERMS, bool IDENT, bool MULTI>
__global__ __launch_bounds__(256) void gemm_nt_half_kernel(const GemmNTArgs a) {
  static_assert(TERMS == 1 || TERMS == 3, "1 or 3 products");
  constexpr int BM = HBM, BN = 64 * TNB, TM = 2, TN = TNB;
  constexpr int NP = TERMS == 3 ? 2 : 1;                  // operand parts held: hi (and lo)
  constexpr int GA = BM / 64, GB = BN / 64;               // granules per staging thread and chunk
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* coef = reinterpret_cast<float4*>(smem);                                             // [sln_crows(K)] (affine operands)
  _Float16* As = reinterpret_cast<_Float16*>(smem + (IDENT ? 0 : (size_t)sln_crows(a.K) * 16));   // [NP][BM][HLD]
  _Float16* Bs = As + NP * BM * HLD;                                                          // [NP][BN][HLD]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Mr = a.M, Nr = a.N, Kr = a.K;
  const int tiles_n = (Nr + BN - 1) / BN;
  const int lb = xcd_remap(blockIdx.x, ((Mr + BM - 1) / BM) * tiles_n);
  const int m0 = (lb / tiles_n) * BM, n0 = (lb % tiles_n) * BN;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * (32 * TN);

  // staging: thread (r0, kq) owns the granules of rows r0 + 64 p at columns 8 kq .. 8 kq + 7 of the chunk
  const int kq = tid & 3, r0 = tid >> 2;
  int rid[GA], ra_idx[GA], rb_idx[GA];
  const float* rowA[GA];
#pragma unroll
  for (int p = 0; p < GA; ++p) {
    const int row = min(m0 + r0 + 64 * p, Mr - 1);         // clamped: rows behind M are loaded from a valid row and never stored
    ra_idx[p] = a.A.idx_a ? ldi(a.A.idx_a + row) : row;
    rb_idx[p] = a.A.idx_b ? ldi(a.A.idx_b + row) : row;
    const Seg& g = a.A.seg[0];
    rid[p] = MULTI ? row : (g.which == 0 ? row : (g.which == 1 ? ra_idx[p] : rb_idx[p]));
    rowA[p] = g.x1 + (size_t)rid[p] * g.ld1 + g.c1;
  }
  const float* rowB[GB];
#pragma unroll
  for (int p = 0; p < GB; ++p) rowB[p] = a.W + (size_t)min(n0 + r0 + 64 * p, Nr - 1) * a.ldw;

  float4 ga[GA][2], gb[GB][2];
  // every load is unconditional at a clamped (valid) address; the columns behind K of the last chunk are never read from LDS
  auto gload = [&](int kt) {
    const int kc = kt * HBK + 8 * kq;
    if (MULTI) {
      const SegSel sg = pick_seg<2>(a.A, kc, kc);
      const int cs = min(kc, sg.end - 8) - sg.base;
#pragma unroll
      for (int p = 0; p < GA; ++p) {
        const int r = sg.which == 0 ? rid[p] : (sg.which == 1 ? ra_idx[p] : rb_idx[p]);
        const float* src = sg.x1 + (size_t)r * sg.ld1 + sg.c1 + cs;
        ga[p][0] = ld4(src); ga[p][1] = ld4(src + 4);
      }
    } else {
      const int cs = min(kc, Kr - 8);
#pragma unroll
      for (int p = 0; p < GA; ++p) { ga[p][0] = ld4(rowA[p] + cs); ga[p][1] = ld4(rowA[p] + cs + 4); }
    }
    const int cw = min(kc, Kr - 8);
#pragma unroll
    for (int p = 0; p < GB; ++p) { gb[p][0] = ld4(rowB[p] + cw); gb[p][1] = ld4(rowB[p] + cw + 4); }
  };
  auto lstore = [&](int kt) {
    const int kc = min(kt * HBK + 8 * kq, Kr - 8);
    float4 cf[8];
    if (!IDENT) {
#pragma unroll
      for (int j = 0; j < 8; ++j) cf[j] = coef[sln_cidx(kc) + j];       // 8 columns from a multiple of 8: one run of the table
    }
#pragma unroll
    for (int p = 0; p < GA; ++p) {
      const float4 u = IDENT ? ga[p][0] : xform1(ga[p][0], cf);
      const float4 w = IDENT ? ga[p][1] : xform1(ga[p][1], cf + 4);
      f16x8 hi, lo;
      half_split8<TERMS>(u, w, hi, lo);
      _Float16* dst = As + (r0 + 64 * p) * HLD + 8 * kq;
      *reinterpret_cast<f16x8*>(dst) = hi;
      if (TERMS == 3) *reinterpret_cast<f16x8*>(dst + BM * HLD) = lo;
    }
#pragma unroll
    for (int p = 0; p < GB; ++p) {
      f16x8 hi, lo;
      half_split8<TERMS>(gb[p][0], gb[p][1], hi, lo);
      _Float16* dst = Bs + (r0 + 64 * p) * HLD + 8 * kq;
      *reinterpret_cast<f16x8*>(dst) = hi;
      if (TERMS == 3) *reinterpret_cast<f16x8*>(dst + BN * HLD) = lo;
    }
  };

  gload(0);                      // in front of the (dependent) coefficient set-up
  if (!IDENT) sln_fill_coefs<(MULTI ? 3 : 1)>(a.A, coef, tid, 256);

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  bool jv[TN];                   // wave-uniform: the 32-column block lies inside N
  float bias_pre[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    jv[j] = n0 + wn0 + 32 * j < Nr;
    const int col = min(n0 + wn0 + 32 * j + (lane & 31), Nr - 1);
    bias_pre[j] = a.bias ? sln_ldf(a.bias + col) : 0.f;
  }
  __syncthreads();               // coefficient table visible
  lstore(0);
  __syncthreads();

  const int lrow = lane & 31, lk = 8 * (lane >> 5);
  const int nch = (Kr + HBK - 1) / HBK;
  for (int kt = 0; kt < nch; ++kt) {
    if (kt + 1 < nch) gload(kt + 1);
    const int steps = kt * HBK + 16 < Kr ? 2 : 1;
    for (int s = 0; s < steps; ++s) {
      f16x8 fa[NP][TM], fb[NP][TN];
#pragma unroll
      for (int h = 0; h < NP; ++h) {
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[h][i] = *reinterpret_cast<const f16x8*>(As + (h * BM + wm0 + 32 * i + lrow) * HLD + 16 * s + lk);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[h][j] = *reinterpret_cast<const f16x8*>(Bs + (h * BN + wn0 + 32 * j + lrow) * HLD + 16 * s + lk);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if (!jv[j]) continue;
          if (TERMS == 3) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[NP - 1][j], acc[i][j], 0, 0, 0);      // a_hi w_lo
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[NP - 1][i], fb[0][j], acc[i][j], 0, 0, 0);      // a_lo w_hi
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[0][i], fb[0][j], acc[i][j], 0, 0, 0);             // a_hi w_hi
        }
    }
    __syncthreads();             // everyone done reading the buffer
    if (kt + 1 < nch) { lstore(kt + 1); __syncthreads(); }
  }

  // D layout of the 32 x 32 MFMA: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* Yp = a.Y + a.ycol0;
  const int ldy = a.ldy;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if (!jv[j]) continue;
      const int col = n0 + wn0 + 32 * j + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < Mr) Yp[(size_t)row * ldy + col] = acc[i][j][r] + bias_pre[j];
      }
    }
}

size_t half_smem_bytes(int K, int tnb, int terms, bool ident) {
  return (ident ? 0 : (size_t)sln_crows(K) * 16) + (size_t)(terms == 3 ? 2 : 1) * (HBM + 64 * tnb) * HLD * sizeof(_Float16);
}

// 128-column tiles unless 64-column tiles leave fewer idle columns (N = 64, 192, ...)
int half_tnb(int N) { return sln_cdiv(N, 64) * 64 < sln_cdiv(N, 128) * 128 ? 1 : 2; }

template <int TNB, int TERMS, bool IDENT, bool MULTI>
int launch_half(const GemmNTArgs& a, hipStream_t st) {
  const size_t smem = half_smem_bytes(a.K, TNB, TERMS, IDENT);
  const int grid = sln_cdiv(a.M, HBM) * sln_cdiv(a.N, 64 * TNB);
  if (grid <= 0) return 0;
  if (smem > 48 * 1024) {        // raised once per instantiation (an attribute of the function, not a stream operation)
    static bool raised = false;
    if (!raised) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_half_kernel<TNB, TERMS, IDENT, MULTI>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) return (int)e;
      raised = true;
    }
  }
  hipLaunchKernelGGL((gemm_nt_half_kernel<TNB, TERMS, IDENT, MULTI>), dim3(grid), dim3(256), smem, st, a);
  SLN_CHECK_LAUNCH();
  return 0;
}

template <int TNB, int TERMS>
int launch_half_form(const GemmNTArgs& a, bool ident, bool multi, hipStream_t st) {
  if (ident) return multi ? launch_half<TNB, TERMS, true, true>(a, st) : launch_half<TNB, TERMS, true, false>(a, st);
  return multi ? launch_half<TNB, TERMS, false, true>(a, st) : launch_half<TNB, TERMS, false, false>(a, st);
}

}  // namespace

// Host only, no device access.  M plays no part: a layout decoded alone takes the route of the same layout inside 20 000.
bool sln_nt_half_takes(const GemmNTArgs& a, int epi) {
  if (epi != EPI_PLAIN || a.addend != nullptr) return false;
  if (a.N <= 0 || a.K <= 0 || a.N % 32 != 0 || a.K % 16 != 0 || a.K > HK_MAX) return false;
  if (a.A.nseg < 1 || a.A.nseg > 3) return false;
  int tot = 0;
  for (int s = 0; s < a.A.nseg; ++s) {
    const Seg& g = a.A.seg[s];
    if (g.x2 != nullptr || g.len <= 0 || g.len % 16 != 0) return false;
    if (g.coef != SLN_COEF_IDENT && g.coef != SLN_COEF_FWD && g.coef != SLN_COEF_FWD_NORELU) return false;
    tot += g.len;
  }
  if (tot != a.K) return false;
  return a.ldy % 4 == 0 && a.ycol0 % 4 == 0;
}

int sln_launch_gemm_nt_half(const GemmNTArgs& a, int terms, hipStream_t st) {
  if ((terms != 1 && terms != 3) || !sln_nt_half_takes(a, EPI_PLAIN)) return -2;      // SLN_E_UNSUPPORTED
  SlnProfScope prof(SLN_FAM_GEMM_NT, 2.0 * a.M * a.N * a.K, st);
  const bool ident = nt_amode(a) == 2, multi = a.A.nseg > 1;
  static const bool nt_log = std::getenv("SLN_NT_LOG") != nullptr;                      // as sln_launch_gemm_nt, with the product count
  if (nt_log) std::fprintf(stderr, "NTLOG M=%d N=%d K=%d amode=%d epi=%d nseg=%d half=%d\n", a.M, a.N, a.K, ident ? 2 : 0, EPI_PLAIN, a.A.nseg, terms);
  if (half_tnb(a.N) == 1) return terms == 3 ? launch_half_form<1, 3>(a, ident, multi, st) : launch_half_form<1, 1>(a, ident, multi, st);
  return terms == 3 ? launch_half_form<2, 3>(a, ident, multi, st) : launch_half_form<2, 1>(a, ident, multi, st);
}
