// Rotated-cuboid IoU of layouts (testing/test_render_refine.py:78-116 get_boxes, testing/test_utils.py:7-40 get_eight_coors_bbox_new /
// get_iou_cuboid, the commented-out print_iou block :360-368) and the interpenetration of a layout's own furniture.
//
//   corners   box * room extent (the room row's [3:6], :90-91), centred, rotated about y by theta = -angle * (2 pi / 24) with
//             [[c, 0, s], [0, 1, 0], [-s, 0, c]] (:98-106), translated back; ring (min, min_max, max, max_min) in (x, z); heights y0, y1
//   iou       inter2d * max(0, min(h1a, h1b) - max(h0a, h0b)) / (vol_a + vol_b - inter + 1e-5), vol = area * (h1 - h0) (signed height)
//
// The reference hands the rings to shapely: areas are unsigned and the winding of a ring does not matter (a decoder may predict
// x1 < x0).  Here: both quads are brought to counter-clockwise order (sign of the shoelace sum), quad a is clipped against the four
// edges of quad b (Sutherland-Hodgman) and the shoelace sum of what is left is taken.  The polygon (at most 8 vertices) lives in
// registers: every index below is a compile-time constant after unrolling, a vertex is appended through a select per slot.
// float32 throughout, contraction off (build.py): theta and the rotation are formed as :100-106 forms them.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "layout_geom.h"
#include "sln_common.h"
#include "sln_hip.h"

namespace {

constexpr int QV = 8;                     // vertices of quad ^ quad: each of the 4 clips adds at most one

// area of quad a ^ quad b (convex, any winding, possibly degenerate); NaN coordinates end with an empty polygon (every comparison
// false): 0, and the caller's volumes carry the NaN
__device__ __forceinline__ float quad_intersection_area(const float2 a[4], const float2 b[4]) {
  const bool fa = shoelace4(a) < 0.f, fb = shoelace4(b) < 0.f;
  float px[QV], py[QV];
  int n = 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const float2 v = a[(fa && (k & 1)) ? (k ^ 2) : k]; px[k] = v.x; py[k] = v.y; }
#pragma unroll
  for (int k = 4; k < QV; ++k) { px[k] = 0.f; py[k] = 0.f; }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int e0 = (fb && (e & 1)) ? (e ^ 2) : e, e1n = (e + 1) & 3, e1 = (fb && (e1n & 1)) ? (e1n ^ 2) : e1n;
    const float bx = b[e0].x, by = b[e0].y, ex = b[e1].x - bx, ey = b[e1].y - by;
    float d[QV];
#pragma unroll
    for (int k = 0; k < QV; ++k) d[k] = ex * (py[k] - by) - ey * (px[k] - bx);        // >= 0: on the inner side of edge e
    float ox[QV], oy[QV];
#pragma unroll
    for (int k = 0; k < QV; ++k) { ox[k] = 0.f; oy[k] = 0.f; }
    int m = 0;
#pragma unroll
    for (int k = 0; k < QV; ++k) {
      const bool wrap = k + 1 >= n;                                                  // the successor of the last vertex is vertex 0
      const float cx = px[k], cy = py[k], dc = d[k];
      const float nx = (k + 1 < QV && !wrap) ? px[(k + 1) % QV] : px[0], ny = (k + 1 < QV && !wrap) ? py[(k + 1) % QV] : py[0];
      const float dn = (k + 1 < QV && !wrap) ? d[(k + 1) % QV] : d[0];
      const bool live = k < n, in_c = dc >= 0.f, in_n = dn >= 0.f;
      const bool put_c = live && in_c, put_x = live && (in_c != in_n) && (dc == dc) && (dn == dn);
      const float t = dc / (dc - dn);
      const float ix = cx + t * (nx - cx), iy = cy + t * (ny - cy);
#pragma unroll
      for (int s = 0; s < QV; ++s) { const bool w = put_c && s == m; ox[s] = w ? cx : ox[s]; oy[s] = w ? cy : oy[s]; }
      m += put_c ? 1 : 0;
#pragma unroll
      for (int s = 0; s < QV; ++s) { const bool w = put_x && s == m; ox[s] = w ? ix : ox[s]; oy[s] = w ? iy : oy[s]; }
      m += put_x ? 1 : 0;
    }
    n = m < QV ? m : QV;                                                             // (a ninth vertex can only be rounding noise: dropped)
#pragma unroll
    for (int k = 0; k < QV; ++k) { px[k] = ox[k]; py[k] = oy[k]; }
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < QV; ++k) {
    const bool wrap = k + 1 >= n;
    const float nx = (k + 1 < QV && !wrap) ? px[(k + 1) % QV] : px[0], ny = (k + 1 < QV && !wrap) ? py[(k + 1) % QV] : py[0];
    s += k < n ? px[k] * ny - nx * py[k] : 0.f;
  }
  return fabsf(0.5f * s);
}

__device__ __forceinline__ float cuboid_pair(const Cuboid& a, const Cuboid& b, float* inter_vol) {
  const float inter2d = quad_intersection_area(a.c, b.c);
  const float inter = inter2d * fmaxf(0.f, fminf(a.h1, b.h1) - fmaxf(a.h0, b.h0));
  const float va = fabsf(shoelace4(a.c)) * (a.h1 - a.h0), vb = fabsf(shoelace4(b.c)) * (b.h1 - b.h0);
  *inter_vol = inter;
  return inter / (va + vb - inter + 1e-5f);
}

// One lane per (layout, row).  The mean of a room is formed by the lane of its room row - the last row of the room - over the room's
// rows in ascending order (fp64): the rows inside this workgroup from LDS, those in front of it (a room that straddles the block
// boundary) recomputed.  One writer per (layout, room), fixed order: bit-identical run to run.
constexpr int IOU_BLOCK = 256;
__global__ __launch_bounds__(IOU_BLOCK) void cuboid_iou_kernel(const float* __restrict__ boxes, const float* __restrict__ angles,
                                                               const float* __restrict__ gt_boxes, const float* __restrict__ gt_angles,
                                                               const int* __restrict__ room_of_row, const unsigned char* __restrict__ visible,
                                                               const int* __restrict__ room_id, const int n_rooms, const int O,
                                                               float* __restrict__ iou_out, double* __restrict__ mean_out) {
  __shared__ float sh_iou[IOU_BLOCK];
  const int s = blockIdx.y, i0 = blockIdx.x * IOU_BLOCK, i = i0 + threadIdx.x;
  const float* L = boxes + (size_t)s * O * 6;
  const float* A = angles + (size_t)s * O;
  auto row_iou = [&](int j, int rr) -> float {
    const Cuboid p = make_cuboid(L + (size_t)j * 6, L + (size_t)rr * 6 + 3, A[j]);
    const Cuboid g = make_cuboid(gt_boxes + (size_t)j * 6, gt_boxes + (size_t)rr * 6 + 3, gt_angles[j]);
    float iv;
    return cuboid_pair(g, p, &iv);
  };
  int rr = -1;
  float v = 0.f;
  if (i < O) {
    rr = room_row_of(room_of_row, i, O);
    if (rr >= 0) v = row_iou(i, rr);
    if (iou_out != nullptr) iou_out[(size_t)s * O + i] = rr >= 0 ? v : __builtin_nanf("");
  }
  sh_iou[threadIdx.x] = v;
  __syncthreads();
  if (mean_out == nullptr || i >= O || rr != i) return;
  const int id = room_id[i];
  if (id < 0 || id >= n_rooms) return;
  int first = i;
  while (first > 0 && room_of_row[first - 1] == i) --first;
  double acc = 0.0;
  long cnt = 0;
  for (int j = first; j <= i; ++j) {
    if (!visible[j]) continue;
    acc += (double)(j >= i0 ? sh_iou[j - i0] : row_iou(j, i));
    ++cnt;
  }
  mean_out[(size_t)s * n_rooms + id] += cnt ? acc / (double)cnt : (double)__builtin_nanf("");       // np.mean([]) is nan
}

// Interpenetration of a layout: over the unordered pairs (i < j) of visible rows of one room, the sum of the intersection volumes
// and the number of pairs whose IoU exceeds thresh.  A group of G lanes (G = 256, or the power of two that holds O rows when O <= 128:
// 256 / G layouts per workgroup) owns a layout: the rows' cuboids are built once into LDS (tiles of whole rooms, OV_CAP rows), lane
// `row` walks its partners j in (row, room row] - O x room size pair tests, nothing O x O anywhere.  fp64 / int64 sums per lane in
// partner order, then a fixed tree over the group.
constexpr int OV_BLOCK = 256, OV_CAP = 1024;
__global__ __launch_bounds__(OV_BLOCK) void layout_overlap_kernel(const float* __restrict__ boxes, const float* __restrict__ angles,
                                                                  const int* __restrict__ room_of_row, const unsigned char* __restrict__ visible,
                                                                  const int S, const int O, const int G, const float thresh,
                                                                  double* __restrict__ vol_out, long long* __restrict__ pairs_out) {
  __shared__ float sc[OV_CAP][10];                      // 4 corners (x, z), h0, h1
  __shared__ double red_v[OV_BLOCK];
  __shared__ long long red_n[OV_BLOCK];
  __shared__ int tile_end[OV_BLOCK / 8];
  const int lpb = OV_BLOCK / G, slot = threadIdx.x / G, lane = threadIdx.x % G;
  const int s = blockIdx.x * lpb + slot;
  const bool have = s < S;
  const float* L = boxes + (size_t)(have ? s : 0) * O * 6;
  const float* A = angles + (size_t)(have ? s : 0) * O;
  const int cap = lpb == 1 ? OV_CAP : G;                // LDS rows of this group: [slot * G, slot * G + cap)
  float (*my)[10] = sc + slot * (lpb == 1 ? 0 : G);
  double acc = 0.0;
  long long cnt = 0;
  bool bad = false;                                     // a room of more than OV_CAP rows (or a broken table): NaN, not a hang
  for (int t0 = 0; t0 < O;) {                           // (t0 is uniform over the workgroup: it depends on the tables only)
    // rows [t0, tend) are the whole rooms that fit into [t0, t0 + cap)
    if (lane == 0) tile_end[slot] = min(t0 + cap, O);
    __syncthreads();
    for (int j = t0 + lane; j < min(t0 + cap, O); j += G) {
      const int rr = room_row_of(room_of_row, j, O);
      if (rr < 0 || rr >= t0 + cap) atomicMin(&tile_end[slot], j);
    }
    __syncthreads();
    const int tend = tile_end[slot];
    for (int j = t0 + lane; j < tend; j += G) {
      const int rr = room_row_of(room_of_row, j, O);
      const Cuboid c = make_cuboid(L + (size_t)j * 6, L + (size_t)rr * 6 + 3, A[j]);
#pragma unroll
      for (int k = 0; k < 4; ++k) { my[j - t0][2 * k] = c.c[k].x; my[j - t0][2 * k + 1] = c.c[k].y; }
      my[j - t0][8] = c.h0; my[j - t0][9] = c.h1;
    }
    __syncthreads();
    if (have)
    for (int i = t0 + lane; i < tend; i += G) {
      if (!visible[i]) continue;
      const int rr = room_of_row[i];
      Cuboid a;
#pragma unroll
      for (int k = 0; k < 4; ++k) a.c[k] = make_float2(my[i - t0][2 * k], my[i - t0][2 * k + 1]);
      a.h0 = my[i - t0][8]; a.h1 = my[i - t0][9];
      for (int j = i + 1; j <= rr; ++j) {
        if (!visible[j]) continue;
        Cuboid b;
#pragma unroll
        for (int k = 0; k < 4; ++k) b.c[k] = make_float2(my[j - t0][2 * k], my[j - t0][2 * k + 1]);
        b.h0 = my[j - t0][8]; b.h1 = my[j - t0][9];
        float iv;
        const float iou = cuboid_pair(a, b, &iv);
        acc += (double)iv;
        cnt += iou > thresh ? 1 : 0;
      }
    }
    __syncthreads();
    if (tend <= t0) { bad = true; break; }              // (uniform: tile_end is shared by the group, and every group sees the same tables)
    t0 = tend;
  }
  red_v[threadIdx.x] = acc; red_n[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = G >> 1; o > 0; o >>= 1) {
    if (lane < o) { red_v[threadIdx.x] += red_v[threadIdx.x + o]; red_n[threadIdx.x] += red_n[threadIdx.x + o]; }
    __syncthreads();
  }
  if (have && lane == 0) {
    vol_out[s] += bad ? (double)__builtin_nanf("") : red_v[threadIdx.x];
    pairs_out[s] += red_n[threadIdx.x];
  }
}

}  // namespace

extern "C" int sln_layout_cuboid_iou(const float* boxes, const float* angles, const float* gt_boxes, const float* gt_angles,
                                     const int32_t* room_of_row, const unsigned char* visible, const int32_t* room_id, int n_rooms, int S, int O,
                                     float* iou_out, double* mean_out, void* stream) {
  if (!boxes || !angles || !gt_boxes || !gt_angles || !room_of_row || S < 0 || O < 0 || (!iou_out && !mean_out)) return SLN_E_BADARG;
  if (mean_out && (!visible || !room_id || n_rooms < 1)) return SLN_E_BADARG;
  if (S == 0 || O == 0) return 0;
  if (S > 65535) return SLN_E_BADARG;
  hipLaunchKernelGGL(cuboid_iou_kernel, dim3(sln_cdiv(O, IOU_BLOCK), S), dim3(IOU_BLOCK), 0, static_cast<hipStream_t>(stream), boxes, angles,
                     gt_boxes, gt_angles, room_of_row, visible, room_id, n_rooms, O, iou_out, mean_out);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_layout_overlap(const float* boxes, const float* angles, const int32_t* room_of_row, const unsigned char* visible, int S, int O,
                                  float thresh, double* vol_out, int64_t* pairs_out, void* stream) {
  if (!boxes || !angles || !room_of_row || !visible || !vol_out || !pairs_out || S < 0 || O < 0) return SLN_E_BADARG;
  if (S == 0 || O == 0) return 0;
  int G = OV_BLOCK;
  if (O <= 128) { G = 8; while (G < O) G <<= 1; }
  const int lpb = OV_BLOCK / G;
  hipLaunchKernelGGL(layout_overlap_kernel, dim3(sln_cdiv(S, lpb)), dim3(OV_BLOCK), 0, static_cast<hipStream_t>(stream), boxes, angles, room_of_row,
                     visible, S, O, G, thresh, vol_out, reinterpret_cast<long long*>(pairs_out));
  SLN_CHECK_LAUNCH();
  return 0;
}
