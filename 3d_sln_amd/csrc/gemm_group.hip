// Grouped launches of the fused GEMM family: two NT problems (forward Linears or dgrads) that are mutually independent run
// as ONE grid.  The scene-graph VAE has pairs of identical-shape branches (box / angle posterior heads of the encoder,
// box_net / angle_net of the decoder) whose GEMMs carry 5-15 us of work each under a ~5 us launch floor; grouping them halves
// the number of dispatches of those stages.  (The wgrads of those Linears run in the per-pass launch, sln_launch_gemm_tn_multi.)
// The kernel body is the one of gemm_f32.hip (gemm_bodies.h).
#include "gemm_bodies.h"

namespace {

struct GroupArgs {
  GemmNTArgs nt[2];
  int nt_blocks[2];
};

// the problem descriptions are SEPARATE kernel parameters: as members of one struct parameter hipcc copied them to
// scratch memory (2.6 KB per lane) and the two-source variants ran 4x slower
template <int AMODE, int EPI, bool MULTI, int ST>
// The block counts that decide which problem a workgroup belongs to are LEADING scalar arguments: they arrive in SGPRs with the
// wavefront (kernarg preload, build.py) - as the last member of the argument block they were a scalar-cache miss of their own
// in front of the first field of the chosen problem.
__global__ __launch_bounds__(256) void gemm_group_kernel(const int nt_blocks0, const int nt_blocks1, const GemmNTArgs a0, const GemmNTArgs a1) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int b = blockIdx.x;
  if (b < nt_blocks0) { gemm_nt_body<64, 64, 2, 2, AMODE, EPI, MULTI, false, ST>(a0, b, nt_blocks0, smem); return; }
  b -= nt_blocks0;
  if (b < nt_blocks1) gemm_nt_body<64, 64, 2, 2, AMODE, EPI, MULTI, false, ST>(a1, b, nt_blocks1, smem);
}

template <int AMODE, int EPI, bool MULTI>
int launch_group(const GroupArgs& g, size_t smem, int blocks, hipStream_t st) {
  if (smem > 48 * 1024) { int r = sln_gemm_init(); if (r) return r; }
  if (g_sln_store_policy & SLN_STORE_NT_WT)
    hipLaunchKernelGGL((gemm_group_kernel<AMODE, EPI, MULTI, SLN_ST_WT>), dim3(blocks), dim3(256), smem, st, g.nt_blocks[0], g.nt_blocks[1], g.nt[0], g.nt[1]);
  else
    hipLaunchKernelGGL((gemm_group_kernel<AMODE, EPI, MULTI, SLN_ST_PLAIN>), dim3(blocks), dim3(256), smem, st, g.nt_blocks[0], g.nt_blocks[1], g.nt[0], g.nt[1]);
  SLN_CHECK_LAUNCH();
  return 0;
}

inline bool nt_multi(const GemmNTArgs& a) { return a.A.nseg > 1; }

template <int AMODE, int EPI, bool MULTI>
int raise_lds_limit() {
  int r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_group_kernel<AMODE, EPI, MULTI, SLN_ST_PLAIN>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (!r) r = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_group_kernel<AMODE, EPI, MULTI, SLN_ST_WT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  return r;
}

}  // namespace

// dynamic-LDS limits of every grouped instantiation (called by sln_gemm_init, outside any stream capture)
int sln_gemm_group_init() {
  int r = 0;
#define SLN_G(AM, EP) if (!r) r = raise_lds_limit<AM, EP, false>(); if (!r) r = raise_lds_limit<AM, EP, true>();
  SLN_G(0, EPI_PLAIN) SLN_G(0, EPI_STATS) SLN_G(2, EPI_PLAIN) SLN_G(2, EPI_STATS)      // forward Linears
  SLN_G(0, EPI_MASK) SLN_G(1, EPI_PLAIN) SLN_G(1, EPI_MASK) SLN_G(2, EPI_MASK)         // dgrads
#undef SLN_G
  return r;
}

// nt[n_nt] with epilogues epi[n_nt]; n_nt <= 2.  All problems must be independent of each other.
// Returns SLN_GROUP_FALLBACK (1) without launching when the problems do not fit one grouped kernel (different operand modes
// or epilogues, shapes that want a bigger tile): the caller then launches them one by one.
int sln_launch_gemm_group(const GemmNTArgs* nt, const int* epi, int n_nt, hipStream_t st) {
  if (n_nt < 1 || n_nt > 2) return 1;
  GroupArgs g; std::memset(&g, 0, sizeof(g));
  const int amode = nt_amode(nt[0]);
  bool multi = false;
  double work = 0.0;
  size_t smem = 0;
  int blocks = 0;
  for (int i = 0; i < n_nt; ++i) {
    if (nt[i].M <= 0 || nt[i].N <= 0 || nt_big_shape(nt[i]) || nt_amode(nt[i]) != amode || epi[i] != epi[0]) return 1;
    multi |= nt_multi(nt[i]);
    if (nt_multi(nt[i]) && nt_unaligned(nt[i])) return 1;
    g.nt[i] = nt[i];
    g.nt_blocks[i] = sln_cdiv(nt[i].M, 64) * sln_cdiv(nt[i].N, 64);
    blocks += g.nt_blocks[i];
    const size_t s = nt_smem_bytes(nt[i].K, 64, 64, 2);
    smem = s > smem ? s : smem;
    work += 2.0 * nt[i].M * nt[i].N * nt[i].K;
  }
  if (multi && epi[0] == EPI_MASK) return 1;
  SlnProfScope prof(SLN_FAM_GEMM_DUAL, work, st);
  const int e0 = epi[0];
#define SLN_GROUP(AM, EP)                                                                         \
  if (amode == AM && e0 == EP)                                                                    \
    return multi ? launch_group<AM, EP, true>(g, smem, blocks, st) : launch_group<AM, EP, false>(g, smem, blocks, st);
  SLN_GROUP(0, EPI_PLAIN) SLN_GROUP(0, EPI_STATS) SLN_GROUP(2, EPI_PLAIN) SLN_GROUP(2, EPI_STATS)
  SLN_GROUP(0, EPI_MASK) SLN_GROUP(1, EPI_PLAIN) SLN_GROUP(1, EPI_MASK) SLN_GROUP(2, EPI_MASK)
#undef SLN_GROUP
  return 1;
}
