// Clock stamps of pixel_map_backward_kernel (raster.hip, the only file that includes this one).  The kernel holds one PmbStamp and
// calls a member at each stamp site.  Product build: the struct is empty and so is every member - the kernel's code is the same with
// or without the calls.  Lab build (-DPMB_STAMP): per-workgroup clock sums (prologue, phase 1, phase 2a load waits / evaluation /
// passes / rows, phase 2b), one slot per workgroup, read back by sln_lab_pmb_stamps (tools/lab/pmb_stamps.py).
#pragma once
#include <hip/hip_runtime.h>

#ifdef PMB_STAMP
namespace {
constexpr int PMB_STAMP_SLOTS = 1 << 19;
__device__ unsigned long long g_pmb_stamp[PMB_STAMP_SLOTS][10];      // [8], [9]: wall clock (100 MHz) at the start and the end

struct PmbStamp {
  unsigned long long T_start, W_start, T_pro, T_p1, T_wait, T_eval, T_2b, N_pass, N_rows;
  unsigned long long t0;                                             // the open interval's start
  static __device__ __forceinline__ unsigned long long now() { return (unsigned long long)clock64(); }
  __device__ __forceinline__ void begin() {
    T_start = now(); W_start = (unsigned long long)wall_clock64();
    T_p1 = 0; T_wait = 0; T_eval = 0; T_2b = 0; N_pass = 0; N_rows = 0; T_pro = 0;
  }
  __device__ __forceinline__ void prologue_done() { T_pro = now() - T_start; }
  __device__ __forceinline__ void round_start() { t0 = now(); }
  __device__ __forceinline__ void phase1_done() { T_p1 += now() - t0; }
  __device__ __forceinline__ void row() { ++N_rows; }
  __device__ __forceinline__ void pass_start() { t0 = now(); }
  __device__ __forceinline__ void loads_landed() { const unsigned long long t = now(); T_wait += t - t0; ++N_pass; t0 = t; }
  // (the accumulators pinned: the evaluation's last instructions stay in front of the clock read)
  __device__ __forceinline__ void eval_done(float& acc0, float& acc1) { asm volatile("" : "+v"(acc0), "+v"(acc1)); T_eval += now() - t0; }
  __device__ __forceinline__ void phase2b_start() { t0 = now(); }
  __device__ __forceinline__ void phase2b_done(float& acc0, float& acc1) { asm volatile("" : "+v"(acc0), "+v"(acc1)); T_2b += now() - t0; }
  __device__ __forceinline__ void flush() const {                    // one lane of the workgroup
    unsigned long long* o = g_pmb_stamp[((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) & (PMB_STAMP_SLOTS - 1)];
    o[0] = now() - T_start; o[1] = T_pro; o[2] = T_p1; o[3] = T_wait; o[4] = T_eval; o[5] = N_pass; o[6] = T_2b; o[7] = N_rows;
    o[8] = W_start; o[9] = (unsigned long long)wall_clock64();
  }
};
}  // namespace

extern "C" int sln_lab_pmb_stamps(unsigned long long* host, int clear) {
  if (clear) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_pmb_stamp)) != hipSuccess) return -1; return (int)hipMemset(p, 0, sizeof(g_pmb_stamp)); }
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pmb_stamp), sizeof(g_pmb_stamp));
}
#else
struct PmbStamp {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void prologue_done() {}
  __device__ __forceinline__ void round_start() {}
  __device__ __forceinline__ void phase1_done() {}
  __device__ __forceinline__ void row() {}
  __device__ __forceinline__ void pass_start() {}
  __device__ __forceinline__ void loads_landed() {}
  __device__ __forceinline__ void eval_done(float&, float&) {}
  __device__ __forceinline__ void phase2b_start() {}
  __device__ __forceinline__ void phase2b_done(float&, float&) {}
  __device__ __forceinline__ void flush() const {}
};
#endif
