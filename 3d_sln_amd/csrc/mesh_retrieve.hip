// Mesh retrieval (models/misc.py): suncg_retrieve :34-64, wall_retrieve :123-137, floor_retrieve :139-152 on the device.
//
// For every object row the model of the row's class whose bounding-box edge ratios (y/x, z/x) are nearest (L1, float64) to those of the
// predicted box.  The output is an argmin, so the arithmetic is the reference's operation by operation (this file is compiled with
// -ffp-contract=off and must never see a fast-division flag: `/` below is the correctly rounded IEEE division):
//   fp32: the six box entries times the room row's [3], [4], [5], one multiplication each (:36-42), the three differences (:50-52),
//         the two quotients dy/dx, dz/dx (:53);
//   fp64: |t0 - r0| + |t1 - r1| against the table ratios (:58-60; the table is formed on the host in float64);
//   np.argmin (:62): the first minimum wins, a NaN distance beats everything and the first NaN is kept.
// One row per lane.  The table is staged through LDS in chunks of RT_CHUNK models (32 KiB: no attribute to raise, two blocks per CU);
// a lane walks the part of its class's slice that lies in the staged chunk and carries (best, index) across chunks - `<` keeps an
// earlier chunk's minimum on a tie.  No atomics, nothing read back, no allocation: capturable, on the caller's stream.
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int RT_BLOCK = 256;
constexpr int RT_CHUNK = 2048;                     // models per LDS chunk: 2048 * 2 * 8 bytes = 32 KiB

// np.argmin's update: `d` replaces `best` when nothing is held yet, or when the held value is not a NaN and d is smaller or a NaN.
// Two selects on one predicate, no branch: the walk is a dependent chain either way, and both results provably move together.
__device__ __forceinline__ void argmin_step(double d, int j, double& best, int& at) {
  const bool take = (at < 0) | ((best == best) & ((d < best) | (d != d)));
  best = take ? d : best;
  at = take ? j : at;
}

__global__ void __launch_bounds__(RT_BLOCK) mesh_retrieve_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ room_row,
                                                                const int32_t* __restrict__ objs, const int32_t* __restrict__ class_ptr,
                                                                int n_classes, const double* __restrict__ model_ratio, int M, int N,
                                                                int32_t* __restrict__ choice, double* __restrict__ dist) {
  __shared__ double2 tab[RT_CHUNK];
  const int i = blockIdx.x * RT_BLOCK + threadIdx.x;
  const size_t lay = (size_t)blockIdx.y * (size_t)N;
  int a = 0, b = 0;                                // the class's slice of the table; empty: the lane only helps staging
  double r0 = 0.0, r1 = 0.0;
  if (i < N) {
    const int rr = room_row[i], c = objs[i];
    if (rr >= 0 && rr < N && rr != i && c >= 0 && c < n_classes) {
      a = class_ptr[c]; b = class_ptr[c + 1];
      a = a < 0 ? 0 : a; b = b > M ? M : b;        // (a table that does not describe M models cannot lead outside it)
      const float* bx = boxes + (lay + (size_t)i) * 6;
      const float* rm = boxes + (lay + (size_t)rr) * 6;
      const float ex = rm[3], ey = rm[4], ez = rm[5];
      const float x0 = bx[0] * ex, x1 = bx[3] * ex, y0 = bx[1] * ey, y1 = bx[4] * ey, z0 = bx[2] * ez, z1 = bx[5] * ez;
      const float dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
      r0 = (double)(dy / dx); r1 = (double)(dz / dx);
    }
  }
  double best = 0.0;
  int at = -1;
  for (int c0 = 0; c0 < M; c0 += RT_CHUNK) {
    const int cn = min(RT_CHUNK, M - c0);
    if (c0 > 0) __syncthreads();                   // every lane is done with the previous chunk
    for (int j = threadIdx.x; j < cn; j += RT_BLOCK) tab[j] = reinterpret_cast<const double2*>(model_ratio)[c0 + j];
    __syncthreads();
    const int lo = max(a, c0) - c0, hi = min(b, c0 + cn) - c0;
    for (int j = lo; j < hi; ++j) {
      const double2 t = tab[j];
      argmin_step(fabs(t.x - r0) + fabs(t.y - r1), c0 + j - a, best, at);
    }
  }
  if (i < N) {
    choice[lay + i] = at;
    if (dist) dist[lay + i] = at < 0 ? (double)__builtin_nanf("") : best;
  }
}

// one lane per room: both tables are a few hundred entries that every lane reads at the same address (a broadcast from cache)
__global__ void __launch_bounds__(64) shell_retrieve_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ last_row, int R, int N,
                                                            const double* __restrict__ wall_ratio, const double* __restrict__ floor_ratio,
                                                            int W, int32_t* __restrict__ out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int rr = last_row[r];
  int wall = -1, floor = -1;
  if (rr >= 0 && rr < N) {
    const float* rm = boxes + (size_t)rr * 6;
    const double X = (double)rm[3], Y = (double)rm[4], Z = (double)rm[5];          // .astype("float") first (:124,141), then float64 quotients
    const double q0 = Y / X, q1 = Z / X;
    double bw = 0.0, bf = 0.0;
    for (int j = 0; j < W; ++j) {
      argmin_step(fabs(wall_ratio[2 * j] - q0) + fabs(wall_ratio[2 * j + 1] - q1), j, bw, wall);
      argmin_step(fabs(floor_ratio[j] - q1), j, bf, floor);
    }
  }
  out[2 * r] = wall; out[2 * r + 1] = floor;
}

}  // namespace

extern "C" int sln_mesh_retrieve(const float* boxes, const int32_t* room_row, const int32_t* objs, const int32_t* class_ptr, int n_classes,
                                 const double* model_ratio, int M, int S, int N, int32_t* choice, double* dist, void* stream) {
  if (!boxes || !room_row || !objs || !class_ptr || !choice || n_classes < 0 || M < 0 || S < 0 || N < 0 || (M > 0 && !model_ratio))
    return SLN_E_BADARG;
  if (reinterpret_cast<uintptr_t>(model_ratio) % 16) return SLN_E_BADARG;
  if (S == 0 || N == 0) return 0;
  if (S > 65535) return SLN_E_BADARG;
  hipLaunchKernelGGL(mesh_retrieve_kernel, dim3(sln_cdiv(N, RT_BLOCK), S), dim3(RT_BLOCK), 0, static_cast<hipStream_t>(stream), boxes, room_row,
                     objs, class_ptr, n_classes, model_ratio, M, N, choice, dist);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_shell_retrieve(const float* boxes, const int32_t* last_row, int R, int N, const double* wall_ratio, const double* floor_ratio,
                                  int W, int32_t* out, void* stream) {
  if (!boxes || !last_row || !out || R < 0 || N < 0 || W < 0 || (W > 0 && (!wall_ratio || !floor_ratio))) return SLN_E_BADARG;
  if (R == 0) return 0;
  hipLaunchKernelGGL(shell_retrieve_kernel, dim3(sln_cdiv(R, 64)), dim3(64), 0, static_cast<hipStream_t>(stream), boxes, last_row, R, N,
                     wall_ratio, floor_ratio, W, out);
  SLN_CHECK_LAUNCH();
  return 0;
}
