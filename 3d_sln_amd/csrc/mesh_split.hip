// Splitting long mesh edges (models/misc.py:79,100 call pymesh.split_long_edges_raw(V, F, 0.6) on every model, wall sub-mesh, floor and
// ceiling).  The rule is this project's own (DESIGN §4 "Splitting long edges"; host/mesh_prep.py restates it in numpy and the tests hold
// these kernels to that restatement for EQUALITY), so the arithmetic is fixed operation by operation - this file is compiled with
// -ffp-contract=off:
//   squared length of an edge   (dx*dx + dy*dy) + dz*dz in float64, d = double(a) - double(b) of the float32 coordinates; the squares make
//                               it symmetric in the endpoints, so two faces that share an edge (or whose edges coincide in position
//                               over different indices) agree on the mark;
//   midpoint                    float32((double(a) + double(b)) * 0.5) per coordinate.
// Three launches per pass, a lane per face / new vertex / face; between them the host sorts the keys and scans the counts (torch).
// No atomics, no allocation, nothing read back here; every lane's output depends on its own input only: the same bytes from call to
// call.  Status words are written with plain stores of one constant per word (racing lanes store the same value).
// Nothing is read outside `v`: every index that leads to a read is range-checked in the lane that uses it.
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int MS_BLOCK = 256;

struct P3 { double x, y, z; };

__device__ __forceinline__ P3 load_p(const float* __restrict__ v, int i) {
  const float* p = v + (size_t)i * 3;
  return P3{(double)p[0], (double)p[1], (double)p[2]};
}
__device__ __forceinline__ double edge_sq(const P3& a, const P3& b) {
  const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(MS_BLOCK) mark_kernel(const float* __restrict__ v, int V, const int32_t* __restrict__ f, int F, double thr,
                                                       int32_t* __restrict__ mask, int32_t* __restrict__ count,
                                                       long long* __restrict__ keys, int32_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (i >= (size_t)F) return;
  int c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = f[i * 3 + k];
  const bool ok = c[0] >= 0 && c[0] < V && c[1] >= 0 && c[1] < V && c[2] >= 0 && c[2] < V;
  int m = 0;
  long long key[3] = {-1, -1, -1};
  if (ok) {
    P3 p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = load_p(v, c[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int a = c[k], b = c[(k + 1) % 3];
      if (edge_sq(p[k], p[(k + 1) % 3]) > thr) {
        m |= 1 << k;
        key[k] = ((long long)min(a, b) << 32) | (long long)max(a, b);
      }
    }
  } else {
    status[0] = 1;                                 // the face is copied through unsplit (mask 0)
  }
  mask[i] = m;
  count[i] = 1 + __popc(m);
#pragma unroll
  for (int k = 0; k < 3; ++k) keys[i * 3 + k] = key[k];
}

__global__ void __launch_bounds__(MS_BLOCK) midpoint_kernel(const float* __restrict__ v, int V, const long long* __restrict__ ukeys, int U,
                                                           float* __restrict__ v_new, int32_t* __restrict__ status) {
  const int u = blockIdx.x * MS_BLOCK + threadIdx.x;
  if (u >= U) return;
  const long long key = ukeys[u];
  const long long a = key >> 32, b = key & 0xFFFFFFFFll;
  float* o = v_new + (size_t)u * 3;
  if (key < 0 || a >= V || b >= V) {               // (a key this library did not form: no read, a defined vertex)
    status[1] = 2;
    o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    return;
  }
  const P3 p = load_p(v, (int)a), q = load_p(v, (int)b);
  o[0] = (float)((p.x + q.x) * 0.5);
  o[1] = (float)((p.y + q.y) * 0.5);
  o[2] = (float)((p.z + q.z) * 0.5);
}

__device__ __forceinline__ void put(int32_t* __restrict__ f_out, int32_t* __restrict__ origin_out, size_t at, int a, int b, int c, int o) {
  f_out[at * 3] = a; f_out[at * 3 + 1] = b; f_out[at * 3 + 2] = c;
  origin_out[at] = o;
}

__global__ void __launch_bounds__(MS_BLOCK) emit_kernel(const float* __restrict__ v_out, int V, int U, const int32_t* __restrict__ f,
                                                       const int32_t* __restrict__ origin, const int32_t* __restrict__ mask,
                                                       const long long* __restrict__ offsets, const int32_t* __restrict__ mid, int F,
                                                       int F_out, int32_t* __restrict__ f_out, int32_t* __restrict__ origin_out,
                                                       int32_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (i >= (size_t)F) return;
  const int m = mask[i] & 7;
  const int n = 1 + __popc(m);
  const long long off = offsets[i];
  if (off < 0 || off + n > (long long)F_out) {     // offsets that are not the scan of these counts: nothing written
    status[2] = 4;
    return;
  }
  const size_t at = (size_t)off;
  const int o = origin[i];
  const int c0 = f[i * 3], c1 = f[i * 3 + 1], c2 = f[i * 3 + 2];
  const int m0 = mid[i * 3], m1 = mid[i * 3 + 1], m2 = mid[i * 3 + 2];
  if (m == 0) {
    put(f_out, origin_out, at, c0, c1, c2, o);
  } else if (m == 7) {
    put(f_out, origin_out, at, c0, m0, m2, o);
    put(f_out, origin_out, at + 1, m0, c1, m1, o);
    put(f_out, origin_out, at + 2, m2, m1, c2, o);
    put(f_out, origin_out, at + 3, m0, m1, m2, o);
  } else if (n == 2) {                             // one marked: edge k
    const int k = m == 1 ? 0 : (m == 2 ? 1 : 2);
    const int A = k == 0 ? c0 : (k == 1 ? c1 : c2), B = k == 0 ? c1 : (k == 1 ? c2 : c0), C = k == 0 ? c2 : (k == 1 ? c0 : c1);
    const int M = k == 0 ? m0 : (k == 1 ? m1 : m2);
    put(f_out, origin_out, at, A, M, C, o);
    put(f_out, origin_out, at + 1, M, B, C, o);
  } else {                                         // two marked: edge k is not
    const int k = m == 6 ? 0 : (m == 5 ? 1 : 2);
    const int A = k == 0 ? c0 : (k == 1 ? c1 : c2), B = k == 0 ? c1 : (k == 1 ? c2 : c0), C = k == 0 ? c2 : (k == 1 ? c0 : c1);
    const int M1 = k == 0 ? m1 : (k == 1 ? m2 : m0), M2 = k == 0 ? m2 : (k == 1 ? m0 : m1);
    const int Vn = V + U;
    bool first = true;                             // a tie, and operands that cannot be read, go to A-M1
    if (A >= 0 && A < V && B >= 0 && B < V && M1 >= V && M1 < Vn && M2 >= V && M2 < Vn) {
      const double dA = edge_sq(load_p(v_out, A), load_p(v_out, M1)), dB = edge_sq(load_p(v_out, B), load_p(v_out, M2));
      first = dA <= dB;
    } else {
      status[2] = 4;
    }
    put(f_out, origin_out, at, M2, M1, C, o);
    if (first) {
      put(f_out, origin_out, at + 1, A, B, M1, o);
      put(f_out, origin_out, at + 2, A, M1, M2, o);
    } else {
      put(f_out, origin_out, at + 1, A, B, M2, o);
      put(f_out, origin_out, at + 2, B, M1, M2, o);
    }
  }
}

inline bool split_sizes_ok(int V, int F) { return V >= 1 && F >= 1 && (long long)V + 3ll * (long long)F < (1ll << 31); }

}  // namespace

extern "C" int sln_mesh_split_mark(const float* v, int V, const int32_t* f, int F, double max_edge_sq, int32_t* mask, int32_t* count,
                                   int64_t* keys, int32_t* status, void* stream) {
  if (!v || !f || !mask || !count || !keys || !status || !split_sizes_ok(V, F)) return SLN_E_BADARG;
  if (!(max_edge_sq > 0.0) || !(max_edge_sq <= 1.7976931348623157e308)) return SLN_E_BADARG;      // NaN, <= 0, infinity
  hipLaunchKernelGGL(mark_kernel, dim3((unsigned)sln_cdiv(F, MS_BLOCK)), dim3(MS_BLOCK), 0, static_cast<hipStream_t>(stream), v, V, f, F,
                     max_edge_sq, mask, count, reinterpret_cast<long long*>(keys), status);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_mesh_split_midpoints(const float* v, int V, const int64_t* ukeys, int U, float* v_new, int32_t* status, void* stream) {
  if (!v || !ukeys || !v_new || !status || V < 1 || U < 1 || (long long)V + (long long)U >= (1ll << 31)) return SLN_E_BADARG;
  hipLaunchKernelGGL(midpoint_kernel, dim3((unsigned)sln_cdiv(U, MS_BLOCK)), dim3(MS_BLOCK), 0, static_cast<hipStream_t>(stream), v, V,
                     reinterpret_cast<const long long*>(ukeys), U, v_new, status);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_mesh_split_emit(const float* v_out, int V, int U, const int32_t* f, const int32_t* origin, const int32_t* mask,
                                   const int64_t* offsets, const int32_t* mid, int F, int F_out, int32_t* f_out, int32_t* origin_out,
                                   int32_t* status, void* stream) {
  if (!v_out || !f || !origin || !mask || !offsets || !mid || !f_out || !origin_out || !status) return SLN_E_BADARG;
  if (!split_sizes_ok(V, F) || U < 0 || (long long)V + (long long)U >= (1ll << 31) || F_out < F || (long long)F_out > 4ll * (long long)F)
    return SLN_E_BADARG;
  hipLaunchKernelGGL(emit_kernel, dim3((unsigned)sln_cdiv(F, MS_BLOCK)), dim3(MS_BLOCK), 0, static_cast<hipStream_t>(stream), v_out, V, U, f,
                     origin, mask, reinterpret_cast<const long long*>(offsets), mid, F, F_out, f_out, origin_out, status);
  SLN_CHECK_LAUNCH();
  return 0;
}
