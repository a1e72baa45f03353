// Fused fp32 MFMA GEMM family for the scene-graph VAE (gfx950).
//
// All matmuls of the hot path are tiny-K (<= 640) fp32 products whose operands are *views* of
// stored pre-activations: BatchNorm+ReLU (forward) or the BatchNorm backward formula is applied
// while the tile is staged, the GraphTripleConv gather/concat is a row-indexed segment, and the
// epilogue produces the column statistics the next BatchNorm needs.  v_mfma_f32_32x32x2_f32 is
// exact fp32 (an fmaf chain) so results stay within 1e-4 of the reference without tricks.
//
//   gemm_nt : Y[M,N]  = op(A)[M,K] * W[N,K]^T (+bias)        forward Linear and dgrad (with W^T)
//   gemm_tn : dW[N,K] += op(G)[R,N]^T * op(X)[R,K]            wgrad, split over row chunks
//   gemm_tn_multi : every wgrad of a backward pass in ONE launch (problem table + one item per workgroup in device memory,
//                   XCD-grouped, ~768-row chunks; sln_tn_multi_plan builds the table on the host)
//
//   gemm_nt16 : the same product on 64 x 96 / 64 x 160 tiles of v_mfma_f32_16x16x4_f32 for the widths (N = 384, 640) that leave
//               64 x 64 tiles with a ragged last round of workgroups (nt16_pick)
//   gemm_nt_small : 32 x 32 tiles, K split over the four wavefronts (the object-side Linears: 64-128 tiles of 64 x 64 for 256 CUs)
//
// NT: k-contiguous LDS tiles ([rows][BK + 4]: one ds_read_b128 feeds four MFMAs); TN: one workgroup frame (gemm_bodies.h: TnFrame -
// coordinates, coefficient tables, register stages, staging, epilogue) around one of two compute cores: TnCoreF32 (row-major fp32
// tiles as the rows arrive, the waves split a tile's rows) or TnCoreSplit (operands as three bf16 parts on the 16-bit pipe, the
// *_split_kernel forms below).  Global->LDS staging goes through registers (the BatchNorm / ReLU / gather
// transform happens on the way), double-buffered so one barrier per K tile.  The K loops of the 64 x 64 NT tile, of the 16 x 16
// body and of the wgrad body are written out instruction by instruction (one piece of staging work behind each MFMA): one
// wavefront per SIMD hides nothing behind its own MFMAs (tools/lab/overlap.hip).  NT kernels with a
// coefficient table run 512 threads: wavefronts 4-7 build the table and leave.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include "gemm_bodies.h"
#include "vae_multi.h"
namespace {
// 64 x 64 tiles with a BatchNorm operand or a masked epilogue run with four helper wavefronts (512 threads, see gemm_nt_body)
constexpr bool nt_coef_helpers(int amode, int epi) { return amode != 2 || epi == EPI_MASK; }      // there is a coefficient table to build
template <int BM, int BN, int AMODE, int EPI>
constexpr bool nt_helpers() { return BM == 64 && BN == 64 && nt_coef_helpers(AMODE, EPI); }
template <int BM, int BN, int WM, int WN, int AMODE, int EPI, int MULTI, int ST = 0>
__global__ __launch_bounds__((nt_helpers<BM, BN, AMODE, EPI>() ? 512 : 256)) void gemm_nt_kernel(const GemmNTArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // the grid is exactly the tile count (launch_nt): computed from M and N, which the body needs anyway, instead of read from the
  // dispatch packet's block count - one kernel-argument cache line less in front of the first address
  gemm_nt_body<BM, BN, WM, WN, AMODE, EPI, MULTI, nt_helpers<BM, BN, AMODE, EPI>(), ST>(a, blockIdx.x, ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN), smem);
}

template <int AMODE, int EPI>
constexpr bool nt_helpers2() { return nt_coef_helpers(AMODE, EPI); }
template <int J, int AMODE, int EPI, int ST = 0>
__global__ __launch_bounds__((nt_helpers2<AMODE, EPI>() ? 512 : 256)) void gemm_nt16_kernel(const GemmNTArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_nt_body16<J, AMODE, EPI, nt_helpers2<AMODE, EPI>(), ST>(a, blockIdx.x, ((a.M + 63) / 64) * ((a.N + 32 * J - 1) / (32 * J)), smem);
}

template <int AMODE, int EPI, int NSEG = 1, int ST = 0>
__global__ __launch_bounds__((nt_helpers2<AMODE, EPI>() ? 512 : 256)) void gemm_nt_small_kernel(const GemmNTArgs a, const int xcd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_nt_small_body<AMODE, EPI, nt_helpers2<AMODE, EPI>(), NSEG, ST>(a, blockIdx.x, smem, xcd != 0);
}

// Forward Linears / dgrads of R rooms (R parameter copies) in one grid: blockIdx.y = room, the room's problem comes out of a device
// table, workgroups beyond its tile count leave (vae_multi.h).  Plain tile order inside a room (a room is a handful of tiles).
template <int AMODE, int EPI, int NSEG>
__global__ __launch_bounds__((nt_helpers2<AMODE, EPI>() ? 512 : 256)) void gemm_nt_small_multi_kernel(const GemmNTArgs* __restrict__ tab, const int* __restrict__ tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int r = blockIdx.y;
  if ((int)blockIdx.x >= tiles[r]) return;
  gemm_nt_small_body<AMODE, EPI, nt_helpers2<AMODE, EPI>(), NSEG>(tab[r], blockIdx.x, smem, false);
}
// ... and of the 64 x 64 body, for the operands the small body does not take (box_net's two-segment input [obj_vecs | attr_emb[attrs]])
template <int AMODE, int EPI, int MULTI>
__global__ __launch_bounds__((nt_helpers<64, 64, AMODE, EPI>() ? 512 : 256)) void gemm_nt64_multi_kernel(const GemmNTArgs* __restrict__ tab, const int* __restrict__ tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int r = blockIdx.y;
  const int nt = tiles[r];
  if ((int)blockIdx.x >= nt) return;
  gemm_nt_body<64, 64, 2, 2, AMODE, EPI, MULTI, nt_helpers<64, 64, AMODE, EPI>()>(tab[r], blockIdx.x, nt, smem);
}

}  // namespace
int sln_gemm_init();
namespace {

// Which kernel an NT launch runs: decided in ONE place (nt_route), carried out by the launchers below.  A launcher whose compiled
// workgroup size differs from the route's refuses to launch, so what sln_debug_gemm_nt_route reports is what runs.
enum { NT_BODY_64 = 0, NT_BODY_128x64 = 1, NT_BODY_128 = 2, NT_BODY_16J3 = 3, NT_BODY_16J5 = 4, NT_BODY_SMALL = 5, NT_BODY_SMALL3 = 6 };
struct NtRoute { int body, multi, amode, threads; };      // multi: 0 one segment, 1 boundaries on k-tiles, 2 a boundary inside a k-tile
// the store form of a launch's epilogue, from the process-wide policy word (sln_common.h)
inline int nt_store_mode() { return (g_sln_store_policy & SLN_STORE_NT_WT) ? SLN_ST_WT : SLN_ST_PLAIN; }

template <int AMODE, int EPI, int NSEG = 1>
int launch_nt_small(const GemmNTArgs& a, const NtRoute& rt, hipStream_t st) {
  if (rt.threads != (nt_helpers2<AMODE, EPI>() ? 512 : 256)) return -3;
  const size_t smem = nt_small_smem_bytes(a.K);
  const int grid = sln_cdiv(a.M, 32) * sln_cdiv(a.N, 32);
  if (grid <= 0) return 0;
  if (smem > 48 * 1024) { int r = sln_gemm_init(); if (r) return r; }
  static const int xcd = std::getenv("SLN_NT_SMALL_NO_XCD") ? 0 : 1;      // lab switch: plain workgroup order
  if (nt_store_mode() == SLN_ST_WT) hipLaunchKernelGGL((gemm_nt_small_kernel<AMODE, EPI, NSEG, SLN_ST_WT>), dim3(grid), dim3(nt_helpers2<AMODE, EPI>() ? 512 : 256), smem, st, a, xcd);
  else hipLaunchKernelGGL((gemm_nt_small_kernel<AMODE, EPI, NSEG>), dim3(grid), dim3(nt_helpers2<AMODE, EPI>() ? 512 : 256), smem, st, a, xcd);
  SLN_CHECK_LAUNCH();
  return 0;
}

template <int J, int AMODE, int EPI>
int launch_nt16(const GemmNTArgs& a, const NtRoute& rt, hipStream_t st) {
  if (rt.threads != (nt_helpers2<AMODE, EPI>() ? 512 : 256)) return -3;
  const size_t smem = nt16_smem_bytes(a.K, J);
  const int grid = sln_cdiv(a.M, 64) * sln_cdiv(a.N, 32 * J);
  if (grid <= 0) return 0;
  if (smem > 48 * 1024) { int r = sln_gemm_init(); if (r) return r; }
  if (nt_store_mode() == SLN_ST_WT) hipLaunchKernelGGL((gemm_nt16_kernel<J, AMODE, EPI, SLN_ST_WT>), dim3(grid), dim3(nt_helpers2<AMODE, EPI>() ? 512 : 256), smem, st, a);
  else hipLaunchKernelGGL((gemm_nt16_kernel<J, AMODE, EPI>), dim3(grid), dim3(nt_helpers2<AMODE, EPI>() ? 512 : 256), smem, st, a);
  SLN_CHECK_LAUNCH();
  return 0;
}

template <int BM, int BN, int WM, int WN, int AMODE, int EPI>
int launch_nt(const GemmNTArgs& a, const NtRoute& rt, hipStream_t st) {
  const size_t smem = nt_smem_bytes(a.K, BM, BN, WM);
  const int grid = sln_cdiv(a.M, BM) * sln_cdiv(a.N, BN);
  if (grid <= 0) return 0;
  if (smem > 48 * 1024) { int r = sln_gemm_init(); if (r) return r; }
  constexpr int NTHR = nt_helpers<BM, BN, AMODE, EPI>() ? 512 : 256;
  if (rt.threads != NTHR) return -3;
#define SLN_NT_GO(ST_)                                                                                                                   \
  if (rt.multi == 2) {                                                                                                                   \
    if constexpr (BM == 64 && BN == 64) hipLaunchKernelGGL((gemm_nt_kernel<64, 64, WM, WN, AMODE, EPI, 2, ST_>), dim3(grid), dim3(NTHR), smem, st, a); \
    else return -2;   /* SLN_E_UNSUPPORTED (nt_route forces the 64 x 64 tile for such operands) */                                       \
  }                                                                                                                                      \
  else if (rt.multi == 1) hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, WM, WN, AMODE, EPI, 1, ST_>), dim3(grid), dim3(NTHR), smem, st, a); \
  else hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, WM, WN, AMODE, EPI, 0, ST_>), dim3(grid), dim3(NTHR), smem, st, a);
  if (nt_store_mode() == SLN_ST_WT) { SLN_NT_GO(SLN_ST_WT) } else { SLN_NT_GO(SLN_ST_PLAIN) }
#undef SLN_NT_GO
  SLN_CHECK_LAUNCH();
  return 0;
}

template <int AMODE, int EPI>
int launch_nt_route(const GemmNTArgs& a, const NtRoute& rt, hipStream_t st) {
  switch (rt.body) {
    case NT_BODY_SMALL: return launch_nt_small<AMODE, EPI>(a, rt, st);
    case NT_BODY_SMALL3: return launch_nt_small<AMODE, EPI, 3>(a, rt, st);
    case NT_BODY_16J3: return launch_nt16<3, AMODE, EPI>(a, rt, st);
    case NT_BODY_16J5: return launch_nt16<5, AMODE, EPI>(a, rt, st);
    case NT_BODY_128x64: return launch_nt<128, 64, 2, 2, AMODE, EPI>(a, rt, st);
    case NT_BODY_128: return launch_nt<128, 128, 2, 2, AMODE, EPI>(a, rt, st);
    case NT_BODY_64: return launch_nt<64, 64, 2, 2, AMODE, EPI>(a, rt, st);
    default: return -1;
  }
}

// The dispatcher's decision.  tile: -1 = choose, 0 / 1 / 2 = the 64 x 64 / 128 x 64 / 128 x 128 body.
NtRoute nt_route(const GemmNTArgs& a, int epi, int tile) {
  static const bool no_small = std::getenv("SLN_NO_SMALL_NT") != nullptr;
  NtRoute r;
  r.amode = nt_amode(a); r.multi = 0;
  // stand-alone launches only: a grouped launch (gemm_group.hip) keeps the 64 x 64 body.  Sharing a grid with another problem's
  // blocks, the small body's 4x more workgroups pay 4x the prologues on a busy chip (measured with a wgrad's blocks next to a
  // dgrad's on every CU: 28.8 -> 30.3 us on average)
  if (tile < 0 && !no_small && nt_wants_small(a)) r.body = NT_BODY_SMALL;
  else if (tile < 0 && !no_small && nt_wants_small3(a)) { r.body = NT_BODY_SMALL3; r.multi = 1; }      // the gathered concat of a graph of a few rows
  else {
    // widths that leave 64 x 64 tiles with a ragged last round (N = 640: 2.5 tiles per CU at 64 graphs, N = 384: 1.5) run on
    // 64 x 160 / 64 x 96 tiles of 16 x 16 MFMAs - one workgroup per CU, see gemm_nt_body16
    const int J16 = tile < 0 ? nt16_pick(a) : 0;
    if (J16 == 3) r.body = NT_BODY_16J3;
    else if (J16 == 5) r.body = NT_BODY_16J5;
    else {
      if (tile < 0) tile = nt_heuristic_tile(a);
      const bool unaligned = a.A.nseg > 1 && nt_unaligned(a);
      if (unaligned) tile = 0;        // the per-thread segment choice exists for the 64x64 tile only
      r.body = tile == 1 ? NT_BODY_128x64 : (tile == 2 ? NT_BODY_128 : NT_BODY_64);
      r.multi = a.A.nseg > 1 ? (unaligned ? 2 : 1) : 0;
    }
  }
  const bool big = r.body == NT_BODY_128x64 || r.body == NT_BODY_128;      // no helper wavefronts (nt_helpers)
  r.threads = !big && nt_coef_helpers(r.amode, epi) ? 512 : 256;
  return r;
}

template <bool G_X2, bool XG>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const GemmTNArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_tn_body<G_X2, XG>(a, blockIdx.x, blockIdx.y, smem);
}

// Every wgrad of a backward pass in one grid: workgroup b runs entry b of the item table (problem, output tile, row chunk; see
// TnMultiMeta for the XCD-aware layout) on that problem's description in device memory (uniform address: scalar loads).
template <bool G_X2, bool XG>
__global__ __launch_bounds__(256) void gemm_tn_multi_kernel(const GemmTNArgs* __restrict__ probs, const TnMultiMeta* __restrict__ meta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TnMultiItem it = meta->item[blockIdx.x];
  if (it.prob < 0) return;
  gemm_tn_body<G_X2, XG>(probs[it.prob], it.tile, it.chunk, smem);
}

// ... and of a whole iteration, gathered X rows or not, in one grid (sln_gemm.h: TnMixedMeta): the item says which of the two
// bodies its problem needs.  The branch is uniform over the workgroup; the kernel's registers are the larger body's.
template <bool G_X2>
__global__ __launch_bounds__(256) void gemm_tn_mixed_kernel(const GemmTNArgs* __restrict__ probs, const TnMixedMeta* __restrict__ meta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_tn_mixed_item<G_X2>(probs, meta->item[blockIdx.x], smem);
}

// ---- the same three launches under the split word (sln_common.h): kernels of their own, so that the ones above stay what they were.
// A single problem is decided on the host; the table kernels ask each workgroup's problem (gemm_tn_mixed_item).
template <bool G_X2, bool XG>
__global__ __launch_bounds__(256) void gemm_tn_split_kernel(const GemmTNArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_tn_split_body<G_X2, XG>(a, blockIdx.x, blockIdx.y, smem);
}
template <bool G_X2, bool XG>
__global__ __launch_bounds__(256) void gemm_tn_multi_split_kernel(const GemmTNArgs* __restrict__ probs, const TnMultiMeta* __restrict__ meta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TnMultiItem it = meta->item[blockIdx.x];
  it.xg = XG ? 1 : 0;                          // the per-kind table carries no gather bit: the launch's kind stands for every item
  gemm_tn_mixed_item<G_X2, true>(probs, it, smem);
}
template <bool G_X2>
__global__ __launch_bounds__(256) void gemm_tn_mixed_split_kernel(const GemmTNArgs* __restrict__ probs, const TnMixedMeta* __restrict__ meta) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemm_tn_mixed_item<G_X2, true>(probs, meta->item[blockIdx.x], smem);
}

// The wgrad kernel variants, known in ONE place: for each launch form a function from (split, x2[, xg]) to the instantiation.  The
// launchers launch through the pointer it returns and tn_kernels_init walks the same functions over every argument, so an
// instantiation cannot be launched without its dynamic-LDS limit raised.
// split: the split word is set and the launch may take the split kernel (sln_common.h: sln_tn_split_launch); x2: G carries a second
// source; xg: X rows are gathered.
using TnKernel = void (*)(GemmTNArgs);
using TnMultiKernel = void (*)(const GemmTNArgs*, const TnMultiMeta*);
using TnMixedKernel = void (*)(const GemmTNArgs*, const TnMixedMeta*);
#define SLN_TN_PICK(K) (x2 ? (xg ? &K<true, true> : &K<true, false>) : (xg ? &K<false, true> : &K<false, false>))
TnKernel tn_kernel(bool split, bool x2, bool xg) { return split ? SLN_TN_PICK(gemm_tn_split_kernel) : SLN_TN_PICK(gemm_tn_kernel); }
TnMultiKernel tn_multi_kernel(bool split, bool x2, bool xg) { return split ? SLN_TN_PICK(gemm_tn_multi_split_kernel) : SLN_TN_PICK(gemm_tn_multi_kernel); }
#undef SLN_TN_PICK
TnMixedKernel tn_mixed_kernel(bool split, bool x2) {
  if (split) return x2 ? &gemm_tn_mixed_split_kernel<true> : &gemm_tn_mixed_split_kernel<false>;
  return x2 ? &gemm_tn_mixed_kernel<true> : &gemm_tn_mixed_kernel<false>;
}
int tn_kernels_init() {
  hipError_t e = hipSuccess;
  auto raise = [&e](auto k) { if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); };
  for (int v = 0; v < 8; ++v) {
    const bool split = v & 4, x2 = v & 2, xg = v & 1;
    raise(tn_kernel(split, x2, xg)); raise(tn_multi_kernel(split, x2, xg));
    if (!xg) raise(tn_mixed_kernel(split, x2));
  }
  return (int)e;
}

int launch_tn(const GemmTNArgs& a, bool x2, hipStream_t st) {
  const size_t smem = tn_smem_bytes(TN_T, TN_T);
  const int gx = sln_cdiv(a.Nout, TN_T) * sln_cdiv(a.Kin, TN_T);
  const int gy = sln_cdiv(a.R, a.rows_per_block);
  if (gx <= 0 || gy <= 0) return 0;
  if (!tn_supported(a)) return -1;
  hipLaunchKernelGGL(tn_kernel(sln_tn_split_launch() && tn_split_takes(a), x2, tn_gathers(a)), dim3(gx, gy), dim3(256), smem, st, a);
  SLN_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// Raise the dynamic-LDS limit of every instantiation once (must not happen inside a stream capture).
template <int BM, int BN, int WM, int WN, int ST>
static int init_nt_tile() {
  hipError_t e = hipSuccess;
#define SLN_SET(X2, EPI)                                                                                          \
  if (e == hipSuccess)                                                                                            \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_kernel<BM, BN, WM, WN, X2, EPI, 0, ST>),       \
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                              \
  if (e == hipSuccess)                                                                                            \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_kernel<BM, BN, WM, WN, X2, EPI, 1, ST>),       \
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                              \
  if (e == hipSuccess && BM == 64 && BN == 64)                                                                    \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_kernel<64, 64, WM, WN, X2, EPI, 2, ST>),       \
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  SLN_SET(0, EPI_PLAIN) SLN_SET(0, EPI_STATS) SLN_SET(0, EPI_MASK)
  SLN_SET(1, EPI_PLAIN) SLN_SET(1, EPI_STATS) SLN_SET(1, EPI_MASK)
  SLN_SET(2, EPI_PLAIN) SLN_SET(2, EPI_STATS) SLN_SET(2, EPI_MASK)
#undef SLN_SET
  return (int)e;
}

int sln_gemm_group_init();
int sln_vae_tail_init();      // vae_kernels.hip: the tail launch runs the wgrad body
int sln_gemm_init() {
  static bool done = false;
  if (done) return 0;
  int r = init_nt_tile<64, 64, 2, 2, SLN_ST_PLAIN>();
  if (!r) r = init_nt_tile<64, 64, 2, 2, SLN_ST_WT>();
#define SLN_SET_S(AM, EPI)                                                                                        \
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_small_kernel<AM, EPI, 1>),         \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                  \
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_small_kernel<AM, EPI, 3>),         \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                  \
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_small_kernel<AM, EPI, 1, SLN_ST_WT>), \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                  \
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_small_kernel<AM, EPI, 3, SLN_ST_WT>), \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  SLN_SET_S(0, EPI_PLAIN) SLN_SET_S(0, EPI_STATS) SLN_SET_S(0, EPI_MASK) SLN_SET_S(1, EPI_PLAIN) SLN_SET_S(1, EPI_STATS)
  SLN_SET_S(1, EPI_MASK) SLN_SET_S(2, EPI_PLAIN) SLN_SET_S(2, EPI_STATS) SLN_SET_S(2, EPI_MASK)
#undef SLN_SET_S
#define SLN_SET_16(J, AM, EPI)                                                                                    \
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt16_kernel<J, AM, EPI>),             \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                  \
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt16_kernel<J, AM, EPI, SLN_ST_WT>),  \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
#define SLN_SET_16J(J)                                                                                            \
  SLN_SET_16(J, 0, EPI_PLAIN) SLN_SET_16(J, 0, EPI_STATS) SLN_SET_16(J, 0, EPI_MASK) SLN_SET_16(J, 1, EPI_PLAIN) SLN_SET_16(J, 1, EPI_STATS) \
  SLN_SET_16(J, 1, EPI_MASK) SLN_SET_16(J, 2, EPI_PLAIN) SLN_SET_16(J, 2, EPI_STATS) SLN_SET_16(J, 2, EPI_MASK)
  SLN_SET_16J(3) SLN_SET_16J(5)
#undef SLN_SET_16J
#undef SLN_SET_16
  if (!r) r = init_nt_tile<128, 64, 2, 2, SLN_ST_PLAIN>();
  if (!r) r = init_nt_tile<128, 64, 2, 2, SLN_ST_WT>();
  if (!r) r = init_nt_tile<128, 128, 2, 2, SLN_ST_PLAIN>();
  if (!r) r = init_nt_tile<128, 128, 2, 2, SLN_ST_WT>();
  if (!r) r = tn_kernels_init();
  if (!r) r = sln_gemm_group_init();
  if (!r) r = sln_vae_tail_init();
  done = r == 0;
  return r;
}




int sln_launch_gemm_nt(const GemmNTArgs& a, int epi, int tile, hipStream_t st) {
  SlnProfScope prof(SLN_FAM_GEMM_NT, 2.0 * a.M * a.N * a.K, st);
  const NtRoute rt = nt_route(a, epi, tile);
  // SLN_NT_LOG=1: one line per launch on stderr (tools/lab/nt_by_shape.sh joins them, in order, with a kernel trace)
  static const bool nt_log = std::getenv("SLN_NT_LOG") != nullptr;
  if (nt_log) std::fprintf(stderr, "NTLOG M=%d N=%d K=%d amode=%d epi=%d nseg=%d\n", a.M, a.N, a.K, rt.amode, epi, a.A.nseg);
#define SLN_DISPATCH(AM)                                                              \
  if (rt.amode == AM) {                                                               \
    if (epi == EPI_MASK) return launch_nt_route<AM, EPI_MASK>(a, rt, st);             \
    if (epi == EPI_STATS) return launch_nt_route<AM, EPI_STATS>(a, rt, st);           \
    return launch_nt_route<AM, EPI_PLAIN>(a, rt, st);                                 \
  }
  SLN_DISPATCH(0) SLN_DISPATCH(1) SLN_DISPATCH(2)
#undef SLN_DISPATCH
  return -1;
}

// ---- multi-room form of the 32 x 32 split-K body (vae_multi.h) -------------------------------------------------------------
int sln_plan_nt_small(const GemmNTArgs& a, int epi, int* tiles) {
  static const bool no_small = std::getenv("SLN_NO_SMALL_NT") != nullptr;
  if (no_small || a.M <= 0 || a.N <= 0) return -1;
  int nseg = 0;
  const int amode = nt_amode(a);
  if (amode == 1 || epi == EPI_STATS) return -1;    // train-mode BatchNorm: not instantiated (the refinement loop runs in eval mode)
  if (nt_wants_small(a)) nseg = 1;                  // the single-room dispatcher's own rules, in its order (sln_launch_gemm_nt)
  else if (nt_wants_small3(a)) nseg = 3;
  if (nseg) { *tiles = sln_cdiv(a.M, 32) * sln_cdiv(a.N, 32); return amode * 16 + epi * 4 + nseg; }
  if (nt_big_shape(a)) return -1;
  // everything else of a room's size: the 64 x 64 body (key 1000 + ...; last digit: 0 one segment, 1 segments on k-tile
  // boundaries, 2 a boundary inside a k-tile)
  *tiles = sln_cdiv(a.M, 64) * sln_cdiv(a.N, 64);
  return 1000 + amode * 16 + epi * 4 + (a.A.nseg > 1 ? (nt_unaligned(a) ? 2 : 1) : 0);
}

template <int AMODE, int EPI, int NSEG>
static int launch_nt_small_multi(const GemmNTArgs* tab, const int* tiles, int R, int max_tiles, size_t smem, hipStream_t st) {
  static bool raised = false;
  if (smem > 48 * 1024 && !raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt_small_multi_kernel<AMODE, EPI, NSEG>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  hipLaunchKernelGGL((gemm_nt_small_multi_kernel<AMODE, EPI, NSEG>), dim3(max_tiles, R), dim3(nt_helpers2<AMODE, EPI>() ? 512 : 256), smem, st, tab, tiles);
  SLN_CHECK_LAUNCH();
  return 0;
}

template <int AMODE, int EPI, int MULTI>
static int launch_nt64_multi(const GemmNTArgs* tab, const int* tiles, int R, int max_tiles, size_t smem, hipStream_t st) {
  static bool raised = false;
  if (smem > 48 * 1024 && !raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_nt64_multi_kernel<AMODE, EPI, MULTI>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  hipLaunchKernelGGL((gemm_nt64_multi_kernel<AMODE, EPI, MULTI>), dim3(max_tiles, R), dim3(nt_helpers<64, 64, AMODE, EPI>() ? 512 : 256), smem, st, tab, tiles);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_launch_gemm_nt_small_multi(const GemmNTArgs* tab, const int* tiles_dev, int R, int key, int max_tiles, int max_K, double flops,
                                   hipStream_t st) {
  if (R <= 0 || max_tiles <= 0) return 0;
  SlnProfScope prof(SLN_FAM_GEMM_NT, flops, st);
  if (key >= 1000) {
    const size_t smem64 = nt_smem_bytes(max_K, 64, 64, 2);
    const int am = (key - 1000) / 16, ep = ((key - 1000) / 4) % 4, mu = (key - 1000) % 4;
#define SLN_NT64M(AM, EP, MU) if (am == AM && ep == EP && mu == MU) return launch_nt64_multi<AM, EP, MU>(tab, tiles_dev, R, max_tiles, smem64, st);
    SLN_NT64M(0, EPI_PLAIN, 0) SLN_NT64M(0, EPI_PLAIN, 1) SLN_NT64M(0, EPI_PLAIN, 2) SLN_NT64M(0, EPI_MASK, 0) SLN_NT64M(0, EPI_MASK, 1) SLN_NT64M(0, EPI_MASK, 2)
    SLN_NT64M(2, EPI_PLAIN, 0) SLN_NT64M(2, EPI_PLAIN, 1) SLN_NT64M(2, EPI_PLAIN, 2) SLN_NT64M(2, EPI_MASK, 0) SLN_NT64M(2, EPI_MASK, 1) SLN_NT64M(2, EPI_MASK, 2)
#undef SLN_NT64M
    return -1;
  }
  const size_t smem = nt_small_smem_bytes(max_K);
  const int amode = key / 16, epi = (key / 4) % 4, nseg = key % 4;
#define SLN_NTM(AM, EP, NS) if (amode == AM && epi == EP && nseg == NS) return launch_nt_small_multi<AM, EP, NS>(tab, tiles_dev, R, max_tiles, smem, st);
  SLN_NTM(0, EPI_PLAIN, 1) SLN_NTM(0, EPI_PLAIN, 3) SLN_NTM(0, EPI_MASK, 1) SLN_NTM(0, EPI_MASK, 3)
  SLN_NTM(2, EPI_PLAIN, 1) SLN_NTM(2, EPI_PLAIN, 3) SLN_NTM(2, EPI_MASK, 1) SLN_NTM(2, EPI_MASK, 3)
#undef SLN_NTM
  return -1;
}

int sln_launch_gemm_tn(const GemmTNArgs& a0, hipStream_t st) {
  SlnProfScope prof(SLN_FAM_GEMM_TN, 2.0 * a0.R * a0.Nout * a0.Kin, st);
  GemmTNArgs a = a0;
  const bool x2 = tn_prepare(a);
  return launch_tn(a, x2, st);
}

// The planner of both table launches.  mixed: the one launch of a whole iteration (items carry their problem's gather bit, plain
// problems keep their null index arrays, and a list that does not fit max_items at the target chunk length is refused instead of
// given longer chunks - see sln_gemm.h).
static int tn_plan(GemmTNArgs* probs, int n, int max_probs, int max_items, bool mixed, int* nprob, int* nblocks, TnMultiItem* item,
                   int* blocks, bool* x2, bool* xg, double* flops) {
  if (n < 1 || n > max_probs) return -1;
  // rows per block: long chunks (tools/gemm_bench.py: a 256-row block spends as long in its prologue, its first-tile latency and
  // its 64 x 64 atomics as in its 8 tiles - 46 TF at R = 4096 against 79 TF with 1.6 k-row chunks)
  static const int target0 = std::getenv("SLN_TN_MULTI_ROWS") ? std::atoi(std::getenv("SLN_TN_MULTI_ROWS")) : 768;
  static const bool no_xcd = std::getenv("SLN_TN_NO_XCD") != nullptr;           // lab: plain order, no XCD grouping
  bool any_x2 = false, any_xg = false;
  double work = 0.0;
  for (int i = 0; i < n; ++i) {
    const GemmTNArgs& a = probs[i];
    if (a.R <= 0 || a.Nout <= 0 || a.Kin <= 0 || !tn_supported(a)) return -1;
    for (int s = 0; s < a.G.nseg; ++s) any_x2 |= a.G.seg[s].x2 != nullptr;
    any_xg |= tn_gathers(a);
    work += 2.0 * a.R * a.Nout * a.Kin;
  }
  // chunking; the launch must fit the item table (8 XCDs x the longest XCD list): longer chunks for big batches
  struct Group { int prob, chunk, tiles; long cost; };
  std::vector<Group> groups;
  int per_xcd[8];
  std::vector<int> owner;
  // deterministic mode: ONE chunk per problem - every dW / db element then receives exactly one add per launch (onto the zeroed
  // gradient, or onto the previous launch's result in stream order): no sum depends on the arrival order of workgroups
  for (long target = g_sln_deterministic ? (1L << 30) : (target0 > 0 ? target0 : 1024);; target *= 2) {
    groups.clear();
    for (int i = 0; i < n; ++i) {
      GemmTNArgs& a = probs[i];
      const int chunks = sln_cdiv(a.R, (int)(target > a.R ? a.R : target));
      a.rows_per_block = sln_cdiv(sln_cdiv(a.R, chunks), BK) * BK;
      const int tiles = sln_cdiv(a.Nout, 64) * sln_cdiv(a.Kin, 64), nch = sln_cdiv(a.R, a.rows_per_block);
      for (int c = 0; c < nch; ++c) {
        const int rows = (c + 1) * a.rows_per_block <= a.R ? a.rows_per_block : a.R - c * a.rows_per_block;
        groups.push_back(Group{i, c, tiles, (long)tiles * rows});
      }
    }
    // longest processing time first: sort the groups by cost (stable), give each to the XCD with the least work so far
    std::stable_sort(groups.begin(), groups.end(), [](const Group& x, const Group& y) { return x.cost > y.cost; });
    long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int x = 0; x < 8; ++x) per_xcd[x] = 0;
    owner.assign(groups.size(), 0);
    for (size_t g = 0; g < groups.size(); ++g) {
      int best = 0;
      if (no_xcd) best = (int)(g % 8);
      else for (int x = 1; x < 8; ++x) if (load[x] < load[best]) best = x;
      owner[g] = best; load[best] += groups[g].cost; per_xcd[best] += groups[g].tiles;
    }
    int mx = 0;
    for (int x = 0; x < 8; ++x) mx = per_xcd[x] > mx ? per_xcd[x] : mx;
    if (8 * mx <= max_items) break;
    if (mixed || target > (1L << 30)) return -1;
  }
  if (any_xg && !mixed) {        // the index pipeline of the gathering body loads indices unconditionally: every X needs a valid array
    const int* any = nullptr;
    for (int i = 0; i < n; ++i) { if (probs[i].X.idx_a) any = probs[i].X.idx_a; else if (probs[i].X.idx_b) any = probs[i].X.idx_b; }
    for (int i = 0; i < n; ++i) if (!probs[i].X.idx_a && !probs[i].X.idx_b) probs[i].X.idx_a = any;
  }
  int mx = 0;
  for (int x = 0; x < 8; ++x) mx = per_xcd[x] > mx ? per_xcd[x] : mx;
  *nprob = n; *nblocks = 8 * mx;
  std::memset(item, 0, sizeof(TnMultiItem) * (size_t)(8 * mx));      // (a table is used by its prefix only, sln_gemm.h: TnMeta)
  for (int b = 0; b < 8 * mx; ++b) item[b].prob = -1;
  int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t g = 0; g < groups.size(); ++g) {          // cost order: an XCD starts with its longest groups
    const int x = owner[g];
    const int gathers = mixed && tn_gathers(probs[groups[g].prob]) ? 1 : 0;
    for (int t = 0; t < groups[g].tiles; ++t) {
      TnMultiItem& it = item[8 * (fill[x]++) + x];        // the j-th workgroup of XCD x is workgroup 8 j + x of the grid
      it.prob = groups[g].prob; it.tile = t; it.chunk = groups[g].chunk; it.xg = gathers;
    }
  }
  *blocks = 8 * mx; *x2 = any_x2; *xg = any_xg; *flops = work;
  return 0;
}

int sln_tn_multi_plan(GemmTNArgs* probs, int n, TnMultiMeta* meta, int* blocks, bool* x2, bool* xg, double* flops) {
  return tn_plan(probs, n, SLN_TN_MULTI_MAX, SLN_TN_MULTI_ITEMS, false, &meta->nprob, &meta->nblocks, meta->item, blocks, x2, xg, flops);
}

int sln_tn_mixed_plan(GemmTNArgs* probs, int n, TnMixedMeta* meta, int* blocks, bool* x2, double* flops) {
  bool xg = false;
  return tn_plan(probs, n, SLN_TN_MIXED_MAX, SLN_TN_MIXED_ITEMS, true, &meta->nprob, &meta->nblocks, meta->item, blocks, x2, &xg, flops);
}

int sln_launch_gemm_tn_multi(const GemmTNArgs* dev_probs, const TnMultiMeta* dev_meta, int blocks, bool x2, bool xg, double flops,
                             hipStream_t st, bool all_keep_f32) {
  if (blocks <= 0) return 0;
  SlnProfScope prof(SLN_FAM_GEMM_TN, flops, st);
  const size_t smem = tn_smem_bytes(64, 64);
  if (smem > 48 * 1024) { int r = sln_gemm_init(); if (r) return r; }
  hipLaunchKernelGGL(tn_multi_kernel(sln_tn_split_launch() && !all_keep_f32, x2, xg), dim3(blocks), dim3(256), smem, st, dev_probs, dev_meta);
  SLN_CHECK_LAUNCH();
  return 0;
}

int sln_launch_gemm_tn_mixed(const GemmTNArgs* dev_probs, const TnMixedMeta* dev_meta, int blocks, bool x2, double flops, hipStream_t st) {
  if (blocks <= 0) return 0;
  SlnProfScope prof(SLN_FAM_GEMM_TN, flops, st);
  const size_t smem = tn_smem_bytes(64, 64);
  if (smem > 48 * 1024) { int r = sln_gemm_init(); if (r) return r; }
  hipLaunchKernelGGL(tn_mixed_kernel(sln_tn_split_launch(), x2), dim3(blocks), dim3(256), smem, st, dev_probs, dev_meta);
  SLN_CHECK_LAUNCH();
  return 0;
}

// Host-only view of the planner for tests (no device work): problems given by their (rows, outputs, inputs); returns the number
// of workgroups, writes rows_per_block[n] and one (problem, tile, chunk) triple per workgroup (problem < 0: padding).
extern "C" int sln_debug_tn_plan(const int* R, const int* Nout, const int* Kin, int n, int* rows_per_block, int* items, int max_items) {
  if (!R || !Nout || !Kin || !rows_per_block || !items || n < 1 || n > SLN_TN_MULTI_MAX) return -1;
  static thread_local GemmTNArgs probs[SLN_TN_MULTI_MAX];
  static thread_local TnMultiMeta meta;
  std::memset(probs, 0, sizeof(GemmTNArgs) * (size_t)n);
  for (int i = 0; i < n; ++i) {
    probs[i].R = R[i]; probs[i].Nout = Nout[i]; probs[i].Kin = Kin[i];
    probs[i].G.nseg = 1; probs[i].X.nseg = 1; probs[i].lddw = i;          // lddw carries the caller's index through the planner
  }
  int blocks = 0; bool x2 = false, xg = false; double flops = 0.0;
  const int r = sln_tn_multi_plan(probs, n, &meta, &blocks, &x2, &xg, &flops);
  if (r) return r;
  if (blocks > max_items) return -2;
  for (int i = 0; i < n; ++i) rows_per_block[probs[i].lddw] = probs[i].rows_per_block;
  for (int b = 0; b < blocks; ++b) {
    const TnMultiItem& it = meta.item[b];
    items[3 * b] = it.prob < 0 ? -1 : probs[it.prob].lddw; items[3 * b + 1] = it.tile; items[3 * b + 2] = it.chunk;
  }
  return blocks;
}

// ... and of the mixed launch's plan: gathers[i] != 0 marks a problem whose X rows are gathered; items[4 * workgroup] = (problem or
// -1, output tile, row chunk, gather bit).  -1 also when the list does not fit the table at the target chunk length.
extern "C" int sln_debug_tn_plan_mixed(const int* R, const int* Nout, const int* Kin, const int* gathers, int n, int* rows_per_block,
                                       int* items, int max_items) {
  if (!R || !Nout || !Kin || !gathers || !rows_per_block || !items || n < 1 || n > SLN_TN_MIXED_MAX) return -1;
  std::vector<GemmTNArgs> probs((size_t)n);
  std::vector<TnMixedMeta> meta(1);
  std::memset(probs.data(), 0, sizeof(GemmTNArgs) * (size_t)n);
  for (int i = 0; i < n; ++i) {
    probs[i].R = R[i]; probs[i].Nout = Nout[i]; probs[i].Kin = Kin[i];
    probs[i].G.nseg = 1; probs[i].X.nseg = 1; probs[i].X.seg[0].which = gathers[i] ? 1 : 0; probs[i].lddw = i;
  }
  int blocks = 0; bool x2 = false; double flops = 0.0;
  const int r = sln_tn_mixed_plan(probs.data(), n, meta.data(), &blocks, &x2, &flops);
  if (r) return r;
  if (blocks > max_items) return -2;
  for (int i = 0; i < n; ++i) rows_per_block[probs[i].lddw] = probs[i].rows_per_block;
  for (int b = 0; b < blocks; ++b) {
    const TnMultiItem& it = meta[0].item[b];
    items[4 * b] = it.prob < 0 ? -1 : probs[it.prob].lddw; items[4 * b + 1] = it.tile; items[4 * b + 2] = it.chunk; items[4 * b + 3] = it.xg;
  }
  return blocks;
}

// ---- test hooks: an arbitrary operand through the dispatchers above (include/sln_hip.h) ----------------------------------------
#include "sln_debug.h"

// what a BatchNorm view must carry for the coefficients `coef` reads out of it (shared with vae_debug.hip)
bool sln_dbg_bn(const SlnDbgBn& d, int coef, BnView& v) {
  std::memset(&v, 0, sizeof(v));
  v.sums = d.sums; v.gsums = d.gsums; v.gamma = d.gamma; v.beta = d.beta; v.rmean = d.rmean; v.rvar = d.rvar;
  v.cstride = d.cstride; v.mode = d.mode; v.n_rows = d.n_rows; v.eps = d.eps;
  v.rn = 1.0 / (double)(d.n_rows > 0.f ? d.n_rows : 1.f);          // on the host, as the engine does
  if (coef == SLN_COEF_IDENT || d.mode == SLN_BN_NONE) return d.mode >= SLN_BN_NONE && d.mode <= SLN_BN_EVAL;
  const bool bwd = coef == SLN_COEF_BWD;
  if (d.mode == SLN_BN_TRAIN) return d.gamma && d.sums && d.cstride > 0 && d.n_rows >= 1.f && (bwd ? d.gsums != nullptr : d.beta != nullptr);
  if (d.mode == SLN_BN_EVAL) return d.gamma && d.rvar && (bwd || (d.beta && d.rmean));
  return false;
}

namespace {

// gather_ok: whether segments may be row-gathered; x2_ok: whether a second source is read at all; ragged_ok (wgrad operands): the
// last segment may end inside a group of four columns when its rows are stored up to the group's end - the body loads whole
// float4s and the coefficients of columns behind the width are zero (box_net.1's six output columns in rows of eight)
bool dbg_operand(const SlnDbgOperand& d, int rows, int cols, bool gather_ok, bool x2_ok, Operand& op, bool ragged_ok = false) {
  std::memset(&op, 0, sizeof(op));
  if (d.nseg < 1 || d.nseg > 3 || rows <= 0) return false;
  int tot = 0;
  for (int s = 0; s < d.nseg; ++s) {
    const SlnDbgSeg& g = d.seg[s];
    Seg& o = op.seg[s];
    const bool ragged = ragged_ok && s == d.nseg - 1 && (g.len & 3);
    const int len4 = (g.len + 3) & ~3;
    if (!g.x1 || g.len <= 0 || ((g.len & 3) && !ragged)) return false;      // (a boundary inside a k-tile: the MULTI = 2 form, nt_route)
    if ((g.ld1 & 3) || (g.c1 & 3) || g.c1 < 0 || g.ld1 < g.c1 + len4) return false;
    if (g.coef < SLN_COEF_IDENT || g.coef > SLN_COEF_BWD || g.which < 0 || g.which > 2) return false;
    if (g.which && (!gather_ok || !(g.which == 1 ? d.idx_a : d.idx_b))) return false;
    if (g.x2) {
      if (!x2_ok || g.coef != SLN_COEF_BWD || (g.ld2 & 3) || (g.c2 & 3) || g.c2 < 0 || g.ld2 < g.c2 + len4) return false;
    } else if (g.coef == SLN_COEF_BWD && g.bn.mode == SLN_BN_TRAIN) return false;      // p1 multiplies the pre-activation
    if (g.coef == SLN_COEF_BWD && !x2_ok) return false;
    o.x1 = g.x1; o.x2 = g.x2; o.ld1 = g.ld1; o.ld2 = g.ld2; o.c1 = g.c1; o.c2 = g.c2; o.len = g.len; o.which = g.which; o.coef = g.coef;
    if (!sln_dbg_bn(g.bn, g.coef, o.bn)) return false;
    tot += g.len;
  }
  if (tot != cols) return false;
  op.idx_a = d.idx_a; op.idx_b = d.idx_b; op.nseg = d.nseg; op.rows = rows; op.cols = cols;
  return true;
}

bool dbg_nt(const SlnDbgGemmNT& d, GemmNTArgs& a) {
  std::memset(&a, 0, sizeof(a));
  if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.epi < EPI_PLAIN || d.epi > EPI_MASK || d.tile < -1 || d.tile > 2) return false;
  if (!dbg_operand(d.A, d.M, d.K, true, true, a.A)) return false;
  if (!d.W || !d.Y || (d.ldw & 3) || d.ldw < d.K || d.ycol0 < 0 || d.ldy < d.ycol0 + d.N) return false;
  if (d.addend && (d.addcol0 < 0 || d.ldadd < d.addcol0 + d.N)) return false;
  if ((d.epi == EPI_STATS && d.osums) || (d.epi == EPI_MASK && d.ogsums)) { if (d.ocstride < d.N) return false; }
  if (d.epi == EPI_MASK) {
    if (!d.xprev || d.xcol0 < 0 || d.ldx < d.xcol0 + d.N || !sln_dbg_bn(d.obn, SLN_COEF_FWD, a.obn)) return false;
  } else if (!sln_dbg_bn(d.obn, SLN_COEF_IDENT, a.obn)) return false;
  a.W = d.W; a.bias = d.bias; a.Y = d.Y; a.ldy = d.ldy; a.ycol0 = d.ycol0; a.M = d.M; a.N = d.N; a.K = d.K; a.ldw = d.ldw;
  a.addend = d.addend; a.ldadd = d.ldadd; a.addcol0 = d.addcol0; a.osums = d.osums; a.ocstride = d.ocstride;
  a.ldx = d.ldx; a.xcol0 = d.xcol0; a.xprev = d.xprev; a.ogsums = d.ogsums;
  return true;
}

bool dbg_tn(const SlnDbgGemmTN& d, GemmTNArgs& a, bool ragged_ok = false) {
  std::memset(&a, 0, sizeof(a));
  if (d.R <= 0 || d.Nout <= 0 || d.Kin <= 0 || !d.dW || d.lddw < d.Kin) return false;
  if (!dbg_operand(d.G, d.R, d.Nout, false, true, a.G, ragged_ok)) return false;       // the gradient operand is addressed by plain rows
  if (!dbg_operand(d.X, d.R, d.Kin, true, false, a.X, ragged_ok)) return false;        // the input operand has one source
  a.dW = d.dW; a.db = d.db; a.lddw = d.lddw; a.R = d.R; a.Nout = d.Nout; a.Kin = d.Kin;
  a.rows_per_block = d.rows_per_block; a.sgd_step = d.sgd_step;
  return true;
}

}  // namespace

extern "C" int sln_debug_gemm_sizes(int* out, int max) {
  const int sz[6] = {(int)sizeof(SlnDbgBn), (int)sizeof(SlnDbgSeg), (int)sizeof(SlnDbgOperand), (int)sizeof(SlnDbgGemmNT),
                     (int)sizeof(SlnDbgGemmTN), (int)sizeof(SlnDbgNTRoute)};
  for (int i = 0; out && i < 6 && i < max; ++i) out[i] = sz[i];
  return 6;
}

extern "C" int sln_debug_gemm_nt_route(const SlnDbgGemmNT* desc, SlnDbgNTRoute* out) {
  GemmNTArgs a;
  if (!desc || !out || !dbg_nt(*desc, a)) return SLN_E_BADARG;
  const NtRoute rt = nt_route(a, desc->epi, desc->tile);
  out->body = rt.body; out->multi = rt.multi; out->amode = rt.amode; out->threads = rt.threads;
  return 0;
}

extern "C" int sln_debug_gemm_nt(const SlnDbgGemmNT* desc, int n, int* grouped, void* stream) {
  if (!desc || n < 1 || n > 2) return SLN_E_BADARG;
  GemmNTArgs nt[2]; int epi[2] = {0, 0};
  for (int i = 0; i < n; ++i) { if (!dbg_nt(desc[i], nt[i])) return SLN_E_BADARG; epi[i] = desc[i].epi; }
  hipStream_t st = (hipStream_t)stream;
  if (grouped) *grouped = 0;
  if (n == 2) {
    const int r = sln_launch_gemm_group(nt, epi, 2, st);
    if (r != 1) { if (grouped && !r) *grouped = 1; return r; }
  }
  for (int i = 0; i < n; ++i) { const int r = sln_launch_gemm_nt(nt[i], epi[i], desc[i].tile, st); if (r) return r; }
  return 0;
}

// the fp16-MFMA launcher (gemm_half.hip) on a caller-built problem; the predicate alone is host only
extern "C" int sln_debug_gemm_nt_half_takes(const SlnDbgGemmNT* desc) {
  GemmNTArgs a;
  if (!desc || !dbg_nt(*desc, a)) return SLN_E_BADARG;
  return sln_nt_half_takes(a, desc->epi) ? 1 : 0;
}

extern "C" int sln_debug_gemm_nt_half(const SlnDbgGemmNT* desc, int terms, void* stream) {
  GemmNTArgs a;
  if (!desc || (terms != 1 && terms != 3) || !dbg_nt(*desc, a)) return SLN_E_BADARG;
  if (!sln_nt_half_takes(a, desc->epi)) return SLN_E_UNSUPPORTED;
  return sln_launch_gemm_nt_half(a, terms, (hipStream_t)stream);
}

extern "C" int sln_debug_gemm_tn(const SlnDbgGemmTN* desc, int n, int multi, void* stream) {
  if (!desc || n < 1 || n > SLN_TN_MULTI_MAX || (!multi && n != 1)) return SLN_E_BADARG;
  std::vector<GemmTNArgs> probs((size_t)n);
  for (int i = 0; i < n; ++i) if (!dbg_tn(desc[i], probs[(size_t)i])) return SLN_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (!multi) return sln_launch_gemm_tn(probs[0], st);
  if (sln_capturing(st)) return SLN_E_CAPTURE;
  std::vector<TnMultiMeta> meta(1);
  int blocks = 0; bool x2 = false, xg = false; double flops = 0.0;
  if (sln_tn_multi_plan(probs.data(), n, meta.data(), &blocks, &x2, &xg, &flops)) return SLN_E_BADARG;
  GemmTNArgs* dprobs = nullptr; TnMultiMeta* dmeta = nullptr;
  const size_t pbytes = sizeof(GemmTNArgs) * (size_t)n;
  int r = (int)hipMalloc((void**)&dprobs, pbytes);
  if (!r) r = (int)hipMalloc((void**)&dmeta, sizeof(TnMultiMeta));
  if (!r) r = (int)hipMemcpy(dprobs, probs.data(), pbytes, hipMemcpyHostToDevice);
  if (!r) r = (int)hipMemcpy(dmeta, meta.data(), sizeof(TnMultiMeta), hipMemcpyHostToDevice);
  if (!r) r = sln_launch_gemm_tn_multi(dprobs, dmeta, blocks, x2, xg, flops, st);
  const int rs = (int)hipStreamSynchronize(st);         // the table must outlive the launch
  if (!r) r = rs;
  if (dprobs) (void)hipFree(dprobs);
  if (dmeta) (void)hipFree(dmeta);
  return r;
}

// the mixed launch (gathered and plain problems in ONE grid) on caller-built problems, 1 <= n <= SLN_TN_MIXED_MAX; tables as above
extern "C" int sln_debug_gemm_tn_mixed(const SlnDbgGemmTN* desc, int n, void* stream) {
  if (!desc || n < 1 || n > SLN_TN_MIXED_MAX) return SLN_E_BADARG;
  std::vector<GemmTNArgs> probs((size_t)n);
  for (int i = 0; i < n; ++i) if (!dbg_tn(desc[i], probs[(size_t)i], true)) return SLN_E_BADARG;      // (widths as the engine's: any)
  hipStream_t st = (hipStream_t)stream;
  if (sln_capturing(st)) return SLN_E_CAPTURE;
  std::vector<TnMixedMeta> meta(1);
  int blocks = 0; bool x2 = false; double flops = 0.0;
  if (sln_tn_mixed_plan(probs.data(), n, meta.data(), &blocks, &x2, &flops)) return SLN_E_BADARG;
  GemmTNArgs* dprobs = nullptr; TnMixedMeta* dmeta = nullptr;
  const size_t pbytes = sizeof(GemmTNArgs) * (size_t)n, mbytes = offsetof(TnMixedMeta, item) + sizeof(TnMultiItem) * (size_t)blocks;
  int r = (int)hipMalloc((void**)&dprobs, pbytes);
  if (!r) r = (int)hipMalloc((void**)&dmeta, sizeof(TnMixedMeta));
  if (!r) r = (int)hipMemcpy(dprobs, probs.data(), pbytes, hipMemcpyHostToDevice);
  if (!r) r = (int)hipMemcpy(dmeta, meta.data(), mbytes, hipMemcpyHostToDevice);
  if (!r) r = sln_launch_gemm_tn_mixed(dprobs, dmeta, blocks, x2, flops, st);
  const int rs = (int)hipStreamSynchronize(st);         // the table must outlive the launch
  if (!r) r = rs;
  if (dprobs) (void)hipFree(dprobs);
  if (dmeta) (void)hipFree(dmeta);
  return r;
}
