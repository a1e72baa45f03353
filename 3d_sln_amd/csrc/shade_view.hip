// The viewpoint render of render/render_semantic_depth.py::render_test between the placed meshes and the SPADE input:
//
//   view_place_project_kernel   R rooms x V candidate views in one launch: every face slot of a room takes its row's affine (A, tr - formed by
//                               the caller in vectorised fp32 torch), places the three corners of the row's bank model, projects them with the
//                               view's K, R, t as sln_project_faces does and collapses a face that comes nearer than `near` (placement.hip's
//                               rule: shapes stay fixed).  Shell slots read the room's placed shell vertices.
//   view_compose_kernel         from sln_raster_forward's maps: class bytes and depth in image row order (Blender's 1e10 where nothing was
//                               hit), and per workgroup the float64 sum / int64 count of the depths below 1e5;
//   view_compose_final_kernel   the partials of a view, added in a fixed order.
//
// Forward only, no atomics, no allocation.  Every index that comes out of device memory is compared with its range before it is used: a
// value outside makes the slot an empty one (see sln_hip.h for what the host checks before the launch).
// Contraction stays on (no -ffp-contract=off for this unit): the test allows four times the fp32 torch restatement's own error.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr float PROJ_EPS = 1e-9f;          // sln_project_faces' eps as host/neural_renderer.py passes it
constexpr float EMPTY_Z = 1e10f;           // Blender's Z where no surface was hit
constexpr float MEAN_BELOW = 1e5f;         // render_semantic_depth.py:370
constexpr int COMPOSE_BLOCKS = 128;        // partials per view

__device__ __forceinline__ void project_corner(const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ t, float os,
                                               const float p[3], float out[3]) {
  const float x = p[0] * R[0] + p[1] * R[1] + p[2] * R[2] + t[0];
  const float y = p[0] * R[3] + p[1] * R[4] + p[2] * R[5] + t[1];
  const float z = p[0] * R[6] + p[1] * R[7] + p[2] * R[8] + t[2];
  const float xh = x / (z + PROJ_EPS), yh = y / (z + PROJ_EPS);
  const float u = xh * K[0] + yh * K[1] + K[2];
  const float v = os - (xh * K[3] + yh * K[4] + K[5]);
  out[0] = 2.f * (u - os / 2.f) / os;
  out[1] = 2.f * (v - os / 2.f) / os;
  out[2] = z;
}

__global__ __launch_bounds__(256) void view_place_project_kernel(SlnViewPlace d, float* __restrict__ fxyz, unsigned char* __restrict__ flabel) {
  const int F = d.N * d.Fm + d.Fs;
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int rv = blockIdx.y, r = rv / d.V;
  float p[3][3];
  bool live = false;
  unsigned char label = 0;
  if (f < d.N * d.Fm) {
    const int row = r * d.N + f / d.Fm, j = f % d.Fm;
    const int m = d.row_model[row];
    if (m >= 0 && m < d.M) {
      const int v0 = d.voff[m], v1 = d.voff[m + 1], f0 = d.foff[m], f1 = d.foff[m + 1];
      // (the device copies of the tables are compared with the bank's sizes once more: see the header)
      if (v0 >= 0 && v1 <= d.Vtot && v0 < v1 && f0 >= 0 && f1 <= d.Ftot && j < f1 - f0) {
        const int32_t* c = d.bank_f + 3L * (f0 + j);
        const int c0 = c[0], c1 = c[1], c2 = c[2], nv = v1 - v0;
        if (c0 >= 0 && c0 < nv && c1 >= 0 && c1 < nv && c2 >= 0 && c2 < nv) {
          live = true;
          label = d.row_label[row];
          const float* A = d.A + 9L * row;
          const float* tr = d.tr + 3L * row;
          const int ci[3] = {c0, c1, c2};
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const float* mv = d.bank_v + 3L * (v0 + ci[q]);
#pragma unroll
            for (int e = 0; e < 3; ++e) p[q][e] = A[3 * e] * mv[0] + A[3 * e + 1] * mv[1] + A[3 * e + 2] * mv[2] + tr[e];
          }
        }
      }
    }
  } else {
    const int s = f - d.N * d.Fm;
    const int32_t* c = d.shell_f + 3L * s;
    const int c0 = c[0], c1 = c[1], c2 = c[2];
    if (c0 >= 0 && c0 < d.Vs && c1 >= 0 && c1 < d.Vs && c2 >= 0 && c2 < d.Vs) {
      live = true;
      label = d.shell_label[s];
      const int ci[3] = {c0, c1, c2};
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float* sv = d.shell_v + 3L * ((long)r * d.Vs + ci[q]);
        p[q][0] = sv[0]; p[q][1] = sv[1]; p[q][2] = sv[2];
      }
    }
  }
  float o[3][3];
  bool cull = !live;
  if (live) {
    const float* K = d.K + 9L * rv;
    const float* R = d.Rm + 9L * rv;
    const float* t = d.t + 3L * rv;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      project_corner(K, R, t, d.orig_size, p[q], o[q]);
      cull = cull || !(o[q][2] >= d.near);          // (a NaN depth is culled too)
    }
  }
  float* out = fxyz + 9L * ((long)rv * F + f);
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int e = 0; e < 3; ++e) out[3 * q + e] = cull ? 0.f : o[q][e];
  if (rv % d.V == 0) flabel[(long)r * F + f] = label;
}

// 256 lanes: the sum of v over the workgroup in lane 0, always in the same order (shuffle tree per wavefront, then wavefronts 0..3)
template <typename T>
__device__ __forceinline__ T block_sum_256(T v, T* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void view_compose_kernel(const int32_t* __restrict__ fi, const float* __restrict__ depth,
                                                           const unsigned char* __restrict__ flabel, int V, int F, int S,
                                                           unsigned char* __restrict__ labels, float* __restrict__ dout,
                                                           double* __restrict__ psum, long long* __restrict__ pcount) {
  const int b = blockIdx.y;
  const long n = (long)S * S, base = (long)b * n;
  const unsigned char* lab = flabel + (long)(b / V) * F;
  double s = 0.0;
  long long c = 0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)COMPOSE_BLOCKS * 256) {
    const int y = (int)(p / S), x = (int)(p - (long)y * S);
    const int k = fi[base + p];
    const bool hit = k >= 0 && k < F;
    const float z = hit ? depth[base + p] : EMPTY_Z;
    const long q = base + (long)(S - 1 - y) * S + x;        // image rows run downwards
    labels[q] = hit ? lab[k] : (unsigned char)0;
    dout[q] = z;
    if (z < MEAN_BELOW) { s += (double)z; c += 1; }
  }
  __shared__ double red_s[4];
  __shared__ long long red_c[4];
  s = block_sum_256(s, red_s);
  c = block_sum_256(c, red_c);
  if (threadIdx.x == 0) { psum[(long)b * COMPOSE_BLOCKS + blockIdx.x] = s; pcount[(long)b * COMPOSE_BLOCKS + blockIdx.x] = c; }
}

__global__ __launch_bounds__(64) void view_compose_final_kernel(const double* __restrict__ psum, const long long* __restrict__ pcount,
                                                                double* __restrict__ sum, long long* __restrict__ count) {
  const int b = blockIdx.x;
  double s = 0.0;
  long long c = 0;
  for (int i = threadIdx.x; i < COMPOSE_BLOCKS; i += 64) { s += psum[(long)b * COMPOSE_BLOCKS + i]; c += pcount[(long)b * COMPOSE_BLOCKS + i]; }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); c += __shfl_down(c, o, 64); }
  if (threadIdx.x == 0) { sum[b] = s; count[b] = c; }
}

int check_tables(const int32_t* off, int M, int total, int cap) {
  if (off[0] != 0) return SLN_E_BADARG;
  for (int m = 0; m < M; ++m) {
    if (off[m + 1] < off[m] || off[m + 1] > total) return SLN_E_BADARG;
    if (cap >= 0 && off[m + 1] - off[m] > cap) return SLN_E_BADARG;
  }
  return 0;
}

}  // namespace

extern "C" {

int sln_view_place_project(const SlnViewPlace* d, float* faces_xyz, unsigned char* face_label, void* stream) {
  if (!d || !faces_xyz || !face_label) return SLN_E_BADARG;
  if (d->R < 1 || d->V < 1 || d->N < 1 || d->Fm < 1 || d->M < 0 || d->Vtot < 0 || d->Ftot < 0 || d->Vs < 0 || d->Fs < 0) return SLN_E_BADARG;
  if ((long)d->R * d->V > 65535) return SLN_E_BADARG;
  if (!d->A || !d->tr || !d->row_model || !d->row_label || !d->K || !d->Rm || !d->t) return SLN_E_BADARG;
  if (!d->voff || !d->foff || !d->voff_host || !d->foff_host) return SLN_E_BADARG;
  if (d->M > 0 && (!d->bank_v || !d->bank_f)) return SLN_E_BADARG;
  if (d->Fs > 0 && (d->Vs < 1 || !d->shell_v || !d->shell_f || !d->shell_f_host || !d->shell_label)) return SLN_E_BADARG;
  if (!(d->orig_size > 0.f)) return SLN_E_BADARG;
  const long F = (long)d->N * d->Fm + d->Fs;
  if (F > (1L << 24)) return SLN_E_BADARG;
  if (check_tables(d->voff_host, d->M, d->Vtot, -1) || check_tables(d->foff_host, d->M, d->Ftot, d->Fm)) return SLN_E_BADARG;
  for (long i = 0; i < 3L * d->Fs; ++i)
    if (d->shell_f_host[i] < 0 || d->shell_f_host[i] >= d->Vs) return SLN_E_BADARG;
  hipLaunchKernelGGL(view_place_project_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)(d->R * d->V)), dim3(256), 0, (hipStream_t)stream, *d,
                     faces_xyz, face_label);
  SLN_CHECK_LAUNCH();
  return 0;
}

int64_t sln_view_compose_workspace_bytes(int B) {
  if (B < 1 || B > 65535) return SLN_E_BADARG;
  return (int64_t)B * COMPOSE_BLOCKS * (sizeof(double) + sizeof(long long));
}

int sln_view_compose(const int32_t* face_index, const float* depth, const unsigned char* face_label, int B, int V, int F, int S,
                     void* workspace, unsigned char* labels, float* depth_out, double* sum, int64_t* count, void* stream) {
  if (!face_index || !depth || !face_label || !workspace || !labels || !depth_out || !sum || !count) return SLN_E_BADARG;
  if (B < 1 || B > 65535 || V < 1 || B % V != 0 || F < 1 || S < 1 || S > 32768) return SLN_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return SLN_E_BADARG;
  double* psum = static_cast<double*>(workspace);
  long long* pcount = reinterpret_cast<long long*>(psum + (size_t)B * COMPOSE_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(view_compose_kernel, dim3(COMPOSE_BLOCKS, B), dim3(256), 0, st, face_index, depth, face_label, V, F, S, labels, depth_out,
                     psum, pcount);
  hipLaunchKernelGGL(view_compose_final_kernel, dim3(B), dim3(64), 0, st, psum, pcount, sum, reinterpret_cast<long long*>(count));
  SLN_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
