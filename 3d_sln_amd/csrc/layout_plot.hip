// Top-down pictures of layouts (testing/test_plot2d.py:9-141 plot2d) and footprint heat maps, S layouts at a time.
//
//   ring      make_cuboid(box, ext = the room row's box[3:6], angle).c[0..3] in (x, z): the statements of :88-110, which are those of
//             get_boxes (layout_geom.h); float32, contraction off (build.py)
//   image     N x N over [0, 1]^2; the pixel of row r, column c has its centre at x = (c + 0.5) / N, z = (r + 0.5) / N - what the
//             reference's `1 - z` (:124) under matplotlib's y-up axes puts on screen, and the container[rd[2], rd[0]] of the heat map
//   coverage  e_k = (q[k+1].x - q[k].x) (p.z - q[k].z) - (q[k+1].z - q[k].z) (p.x - q[k].x); covered when all four e_k >= 0 or all
//             four <= 0 (either winding, edges inclusive) and the pixel lies in the ring's bounding box (true of every covered pixel;
//             it keeps a rounded e_k == 0 outside the box out).  A ring whose shoelace sum is exactly 0 covers nothing; a NaN coordinate
//             fails every comparison
//   painter   among the drawn rows (rank >= 0) of the room that cover a pixel the greatest (rank, row) wins: the order
//             sorted(zip(current_types, iter_idx)) paints in (:118-126), as a max; nothing covers -> winner -1, the floor's colour
//             (:115-117)
//   counts    counts[o, r, c] += the number of layouts whose ring of row o covers the pixel (rows with rank >= 0)
//
// The kernels know nothing of vocabularies: rank [O] (the class's place in nyu_class_order :25-29, < 0 = not drawn :74,86) and
// rgb [O] (mapped_colors :30-71, r | g << 8 | b << 16) are per-row tables built on the host (host/plot2d.py::plot_tables).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout_geom.h"
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int PLOT_BLOCK = 256, PLOT_TILE = 16;       // a workgroup owns a 16 x 16 tile of pixels
constexpr int PLOT_STAGE = 256;                       // rows of a room staged at once (one per lane); longer rooms go in chunks
constexpr int PLOT_MAX_RANK = 127;                    // key = rank << 24 | row
constexpr unsigned FLOOR_RGB = 152u | 223u << 8 | 138u << 16;

// A staged ring: corners, bounding box (inverted - never hit - for a ring that covers nothing)
struct Ring { float2 q[4]; float x0, x1, z0, z1; };

__device__ __forceinline__ Ring make_ring(const Cuboid& c) {
  Ring g;
#pragma unroll
  for (int k = 0; k < 4; ++k) g.q[k] = c.c[k];
  g.x0 = fminf(fminf(c.c[0].x, c.c[1].x), fminf(c.c[2].x, c.c[3].x)); g.x1 = fmaxf(fmaxf(c.c[0].x, c.c[1].x), fmaxf(c.c[2].x, c.c[3].x));
  g.z0 = fminf(fminf(c.c[0].y, c.c[1].y), fminf(c.c[2].y, c.c[3].y)); g.z1 = fmaxf(fmaxf(c.c[0].y, c.c[1].y), fmaxf(c.c[2].y, c.c[3].y));
  if (shoelace4(c.c) == 0.f) { g.x0 = g.z0 = 2.f; g.x1 = g.z1 = -1.f; }          // (NaN != 0: such a ring fails in covers())
  return g;
}

// (the bounding box is part of the test: both kernels decide a pixel in the same way)
__device__ __forceinline__ bool covers(const float2 q[4], const float bb[4], const float px, const float pz) {
  if (bb[1] < px || bb[0] > px || bb[3] < pz || bb[2] > pz) return false;
  bool pos = true, neg = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float2 a = q[k], b = q[(k + 1) & 3];
    const float e = (b.x - a.x) * (pz - a.y) - (b.y - a.y) * (px - a.x);
    pos = pos && e >= 0.f; neg = neg && e <= 0.f;
  }
  return pos || neg;
}

// grid (pixel tiles, rooms, layouts)
__global__ __launch_bounds__(PLOT_BLOCK) void layout_plot_kernel(const float* __restrict__ boxes, const float* __restrict__ angles,
                                                                 const int* __restrict__ room_of_row, const int* __restrict__ room_id,
                                                                 const int* __restrict__ rank, const unsigned* __restrict__ rgb, const int n_rooms,
                                                                 const int O, const int N, const int vec_store, int* __restrict__ winner,
                                                                 unsigned char* __restrict__ image) {
  __shared__ float sh_q[PLOT_STAGE][8];
  __shared__ float sh_bb[PLOT_STAGE][4];
  __shared__ int sh_key[PLOT_STAGE];
  __shared__ unsigned sh_rgb[PLOT_STAGE];
  __shared__ int sh_range[2];
  __shared__ __attribute__((aligned(4))) unsigned char sh_px[PLOT_TILE * PLOT_TILE * 3];
  const int t = threadIdx.x, room = blockIdx.y, s = blockIdx.z;
  const int tiles_x = (N + PLOT_TILE - 1) / PLOT_TILE, tx = blockIdx.x % tiles_x, tz = blockIdx.x / tiles_x;
  const int c = tx * PLOT_TILE + (t & (PLOT_TILE - 1)), r = tz * PLOT_TILE + (t >> 4);
  const float px = ((float)c + 0.5f) / (float)N, pz = ((float)r + 0.5f) / (float)N;
  // the tile's pixel centres span [tx0, tx1] x [tz0, tz1] (the same expressions as px / pz: the reject below is exact for them)
  const float tx0 = ((float)(tx * PLOT_TILE) + 0.5f) / (float)N, tx1 = ((float)(tx * PLOT_TILE + PLOT_TILE - 1) + 0.5f) / (float)N;
  const float tz0 = ((float)(tz * PLOT_TILE) + 0.5f) / (float)N, tz1 = ((float)(tz * PLOT_TILE + PLOT_TILE - 1) + 0.5f) / (float)N;
  const float* L = boxes + (size_t)s * O * 6;
  const float* A = angles + (size_t)s * O;

  // the room's rows [first, last] (consecutive, as suncg_collate_fn lays them out)
  if (t == 0) { sh_range[0] = O; sh_range[1] = -1; }
  __syncthreads();
  int lo = O, hi = -1;
  for (int j = t; j < O; j += PLOT_BLOCK)
    if (room_id[j] == room) { lo = min(lo, j); hi = max(hi, j); }
  if (hi >= 0) { atomicMin(&sh_range[0], lo); atomicMax(&sh_range[1], hi); }
  __syncthreads();
  const int first = sh_range[0], last = sh_range[1];

  int best = -1;
  unsigned best_rgb = FLOOR_RGB;
  for (int j0 = first; j0 <= last; j0 += PLOT_STAGE) {                     // (uniform over the workgroup)
    const int j = j0 + t;
    int key = -1;
    Ring g;
    g.x0 = g.z0 = 2.f; g.x1 = g.z1 = -1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) g.q[k] = make_float2(0.f, 0.f);
    if (j <= last && room_id[j] == room) {
      const int rk = rank[j], rr = room_row_of(room_of_row, j, O);
      if (rk >= 0 && rr >= 0) {
        g = make_ring(make_cuboid(L + (size_t)j * 6, L + (size_t)rr * 6 + 3, A[j]));
        key = (min(rk, PLOT_MAX_RANK) << 24) | j;
        sh_rgb[t] = rgb != nullptr ? rgb[j] : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { sh_q[t][2 * k] = g.q[k].x; sh_q[t][2 * k + 1] = g.q[k].y; }
    sh_bb[t][0] = g.x0; sh_bb[t][1] = g.x1; sh_bb[t][2] = g.z0; sh_bb[t][3] = g.z1;
    sh_key[t] = key;
    __syncthreads();
    const int n = min(PLOT_STAGE, last - j0 + 1);
    for (int i = 0; i < n; ++i) {                                          // every read below is an LDS broadcast
      const int key_i = sh_key[i];
      const bool near = key_i >= 0 && !(sh_bb[i][1] < tx0 || sh_bb[i][0] > tx1 || sh_bb[i][3] < tz0 || sh_bb[i][2] > tz1);
      if (!__builtin_amdgcn_readfirstlane((int)near)) continue;            // the tile and the ring are the workgroup's: uniform
      float2 q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = make_float2(sh_q[i][2 * k], sh_q[i][2 * k + 1]);
      if (key_i > best && covers(q, sh_bb[i], px, pz)) { best = key_i; best_rgb = sh_rgb[i]; }
    }
    __syncthreads();
  }

  const bool inside = c < N && r < N;
  const size_t plane = ((size_t)s * n_rooms + room) * N * N;
  if (winner != nullptr && inside) winner[plane + (size_t)r * N + c] = best < 0 ? -1 : (best & 0xffffff);
  if (image == nullptr) return;
  unsigned char* img = image + plane * 3;
  if (!vec_store) {
    if (inside) {
      unsigned char* p = img + ((size_t)r * N + c) * 3;
      p[0] = best_rgb & 255u; p[1] = (best_rgb >> 8) & 255u; p[2] = (best_rgb >> 16) & 255u;
    }
    return;
  }
  // N % 4 == 0 and a 4-byte aligned image: a tile row is 3 * cols bytes = whole dwords at a dword boundary
  sh_px[t * 3] = best_rgb & 255u; sh_px[t * 3 + 1] = (best_rgb >> 8) & 255u; sh_px[t * 3 + 2] = (best_rgb >> 16) & 255u;
  __syncthreads();
  constexpr int ROW_DW = PLOT_TILE * 3 / 4;                                // 12 dwords per tile row
  const int row = t / ROW_DW, d = t % ROW_DW, cols = min(PLOT_TILE, N - tx * PLOT_TILE), rz = tz * PLOT_TILE + row;
  if (row < PLOT_TILE && rz < N && d * 4 < cols * 3)
    reinterpret_cast<unsigned*>(img + ((size_t)rz * N + tx * PLOT_TILE) * 3)[d] = reinterpret_cast<const unsigned*>(sh_px)[row * ROW_DW + d];
}

// grid (chunk of layouts, row) - the chunks on x, which has no 65 535 limit.  The chunk's rings of the row are built one per lane into LDS; the lanes then share the pixels of the
// window the chunk's rings can reach, count the covering rings in a register and add the count once.  Integer atomics only: exact,
// the same in any order.
constexpr int FP_BLOCK = 128;
__global__ __launch_bounds__(FP_BLOCK) void layout_footprint_kernel(const float* __restrict__ boxes, const float* __restrict__ angles,
                                                                    const int* __restrict__ room_of_row, const int* __restrict__ rank,
                                                                    const int S, const int O, const int N, int* __restrict__ counts) {
  __shared__ float sh_q[FP_BLOCK][8];
  __shared__ float sh_bb[FP_BLOCK][4];
  __shared__ int sh_win[4];                                                // c0, c1, r0, r1 of the chunk's window
  const int t = threadIdx.x, o = blockIdx.y, s0 = blockIdx.x * FP_BLOCK, s = s0 + t;
  if (rank[o] < 0) return;                                                 // (uniform)
  const int rr = room_row_of(room_of_row, o, O);
  if (rr < 0) return;
  if (t == 0) { sh_win[0] = N; sh_win[1] = -1; sh_win[2] = N; sh_win[3] = -1; }
  __syncthreads();
  Ring g;
  g.x0 = g.z0 = 2.f; g.x1 = g.z1 = -1.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) g.q[k] = make_float2(0.f, 0.f);
  if (s < S) {
    const float* L = boxes + (size_t)s * O * 6;
    g = make_ring(make_cuboid(L + (size_t)o * 6, L + (size_t)rr * 6 + 3, angles[(size_t)s * O + o]));
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { sh_q[t][2 * k] = g.q[k].x; sh_q[t][2 * k + 1] = g.q[k].y; }
  sh_bb[t][0] = g.x0; sh_bb[t][1] = g.x1; sh_bb[t][2] = g.z0; sh_bb[t][3] = g.z1;
  // pixel centres (c + 0.5) / N in [x0, x1] <=> c in [x0 N - 0.5, x1 N - 0.5]; one pixel of margin for the rounding of the products.
  // A NaN bound leaves the window alone (the comparison fails): such a ring covers nothing.
  if (g.x0 <= g.x1 && g.z0 <= g.z1) {
    const float fn = (float)N, cap = fn + 1.f;
    const int c0 = max(0, (int)floorf(fminf(fmaxf(g.x0 * fn - 0.5f, -2.f), cap)) - 1), c1 = min(N - 1, (int)ceilf(fminf(fmaxf(g.x1 * fn - 0.5f, -2.f), cap)) + 1);
    const int r0 = max(0, (int)floorf(fminf(fmaxf(g.z0 * fn - 0.5f, -2.f), cap)) - 1), r1 = min(N - 1, (int)ceilf(fminf(fmaxf(g.z1 * fn - 0.5f, -2.f), cap)) + 1);
    if (c0 <= c1 && r0 <= r1) { atomicMin(&sh_win[0], c0); atomicMax(&sh_win[1], c1); atomicMin(&sh_win[2], r0); atomicMax(&sh_win[3], r1); }
  }
  __syncthreads();
  const int c0 = sh_win[0], c1 = sh_win[1], r0 = sh_win[2], r1 = sh_win[3];
  if (c1 < c0 || r1 < r0) return;
  const int W = c1 - c0 + 1, H = r1 - r0 + 1, n = min(FP_BLOCK, S - s0);
  int* plane = counts + (size_t)o * N * N;
  for (int idx = t; idx < W * H; idx += FP_BLOCK) {
    const int r = r0 + idx / W, c = c0 + idx % W;
    const float px = ((float)c + 0.5f) / (float)N, pz = ((float)r + 0.5f) / (float)N;
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
      float2 q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = make_float2(sh_q[i][2 * k], sh_q[i][2 * k + 1]);
      cnt += covers(q, sh_bb[i], px, pz) ? 1 : 0;
    }
    if (cnt) atomicAdd(&plane[(size_t)r * N + c], cnt);
  }
}

}  // namespace

extern "C" int sln_layout_plot(const float* boxes, const float* angles, const int32_t* room_of_row, const int32_t* room_id, const int32_t* rank,
                               const uint32_t* rgb, int n_rooms, int S, int O, int N, int32_t* winner, unsigned char* image, void* stream) {
  if (!boxes || !angles || !room_of_row || !room_id || !rank || (!winner && !image) || (image && !rgb)) return SLN_E_BADARG;
  if (N < 1 || N > 1024 || S < 0 || S > 65535 || O < 0 || O > (1 << 24) || n_rooms < 0 || n_rooms > 65535) return SLN_E_BADARG;
  if (S == 0 || n_rooms == 0) return 0;
  const int tiles = sln_cdiv(N, PLOT_TILE);
  const int vec_store = (N % 4 == 0 && reinterpret_cast<uintptr_t>(image) % 4 == 0) ? 1 : 0;
  hipLaunchKernelGGL(layout_plot_kernel, dim3(tiles * tiles, n_rooms, S), dim3(PLOT_BLOCK), 0, static_cast<hipStream_t>(stream), boxes, angles,
                     room_of_row, room_id, rank, rgb, n_rooms, O, N, vec_store, winner, image);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_layout_footprint_counts(const float* boxes, const float* angles, const int32_t* room_of_row, const int32_t* rank, int S, int O,
                                           int N, int32_t* counts, void* stream) {
  if (!boxes || !angles || !room_of_row || !rank || !counts) return SLN_E_BADARG;
  if (N < 1 || N > 1024 || S < 0 || O < 0 || O > 65535) return SLN_E_BADARG;
  if (S == 0 || O == 0) return 0;
  hipLaunchKernelGGL(layout_footprint_kernel, dim3(sln_cdiv(S, FP_BLOCK), O), dim3(FP_BLOCK), 0, static_cast<hipStream_t>(stream), boxes, angles,
                     room_of_row, rank, S, O, N, counts);
  SLN_CHECK_LAUNCH();
  return 0;
}
