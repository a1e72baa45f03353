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

// d area(a ^ b) / d a's vertices, b fixed, ADDED to (gx, gy) in a's own vertex order.  Of the boundary of a ^ b only the pieces of a's
// edges inside b move with a's vertices to first order: both rings in counter-clockwise order as quad_intersection_area brings them,
// edge p -> q of a (d = q - p) clipped to the parameter interval [s0, s1] of [0, 1] by b's four half planes (the area function's inside
// rule, >= 0), w = (s1^2 - s0^2) / 2: dA/dp += (d.y, -d.x) ((s1 - s0) - w), dA/dq += (d.y, -d.x) w.  Four line clips per edge, no polygon.
// t = f0 / (f0 - f1) is formed only where the signs differ (the denominator is then not 0); an edge with a NaN edge function is empty.
__device__ __forceinline__ void quad_area_grad(const float2 a[4], const float2 b[4], float gx[4], float gy[4]) {
  const bool fa = shoelace4(a) < 0.f, fb = shoelace4(b) < 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int kn = (k + 1) & 3, kp = (fa && (k & 1)) ? (k ^ 2) : k, kq = (fa && (kn & 1)) ? (kn ^ 2) : kn;
    const float2 p = a[kp], q = a[kq];
    float s0 = 0.f, s1 = 1.f;
    bool empty = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int e0 = (fb && (e & 1)) ? (e ^ 2) : e, e1n = (e + 1) & 3, e1 = (fb && (e1n & 1)) ? (e1n ^ 2) : e1n;
      const float bx = b[e0].x, by = b[e0].y, ex = b[e1].x - bx, ey = b[e1].y - by;
      const float f0 = ex * (p.y - by) - ey * (p.x - bx), f1 = ex * (q.y - by) - ey * (q.x - bx);
      const bool in0 = f0 >= 0.f, in1 = f1 >= 0.f, cross = (in0 != in1) && (f0 == f0) && (f1 == f1);
      const float t = (cross ? f0 : 0.f) / (cross ? f0 - f1 : 1.f);
      s1 = (cross && in0) ? fminf(s1, t) : s1;
      s0 = (cross && !in0) ? fmaxf(s0, t) : s0;
      empty = empty || (!(in0 && in1) && !cross);
    }
    const bool live = !empty && s1 > s0;
    const float w = (s1 * s1 - s0 * s0) / 2.f, cp = live ? (s1 - s0) - w : 0.f, cq = live ? w : 0.f;
    const float nx = q.y - p.y, ny = -(q.x - p.x);
    gx[kp] += nx * cp; gy[kp] += ny * cp;
    gx[kq] += nx * cq; gy[kq] += ny * cq;
  }
}

// The interpenetration of a layout as a loss term: per (layout, room) the sum of the intersection volumes of its colliding pairs (the
// terms of layout_overlap_kernel, bit for bit) and weight * its gradient with respect to every row's box and angle.  The frame is
// layout_overlap_kernel's (G lanes per layout, cuboids staged once in LDS in tiles of whole rooms) with two changes that the cost of
// a pair asked for (a pair is ~9 us of one lane: 109 us for 16 rooms of 13 rows with one lane per row, LAB_NOTES §39):
//   * a tile is closed at the first room boundary at or behind `tile_rows` rows and the tiles of a layout are dealt round robin to the
//     gridDim.y workgroups of its column - every workgroup walks the tile boundaries (they follow from the tables alone), stages and
//     works only its own;
//   * OV_SUB adjacent lanes share a row: sub-lane u takes the partners first + u, first + u + OV_SUB, ... of the row's room, the
//     partial sums meet in a fixed butterfly (__shfl_xor 1, 2), sub-lane 0 owns the row's seven gradient values.
// Every pair is worked twice (once from either row), nothing is atomic, the order is fixed by the tables; the value comes from the
// partners behind the row.  The lane of a room row adds the room's rows in ascending order (fp64, from LDS): one writer per
// (layout, room).  The extent (the room row's [3:6]) is a constant here, a room row's gradient is exactly 0.
constexpr int OV_SUB = 4;
__global__ __launch_bounds__(OV_BLOCK) void layout_overlap_penalty_kernel(const float* __restrict__ boxes, const float* __restrict__ angles,
                                                                          const int* __restrict__ room_of_row,
                                                                          const unsigned char* __restrict__ collide,
                                                                          const int* __restrict__ room_id, const int n_rooms, const int S, const int O,
                                                                          const int G, const int tile_rows, const float weight, const int accumulate,
                                                                          double* __restrict__ penalty_out, float* __restrict__ grad_boxes,
                                                                          float* __restrict__ grad_angles) {
  __shared__ float sc[OV_CAP][10];                      // 4 corners (x, z), h0, h1
  __shared__ double row_v[OV_CAP];                      // a row's sum over its partners behind it
  __shared__ int sh_rr[OV_CAP];                         // room_of_row of the tile
  __shared__ int tile_end[OV_BLOCK / 8];
  const int lpb = OV_BLOCK / G, slot = threadIdx.x / G, lane = threadIdx.x % G;
  const int sub = lane % OV_SUB, row_slot = lane / OV_SUB, rows_per_pass = G / OV_SUB;
  const int s = blockIdx.x * lpb + slot;
  const bool have = s < S;
  const float* L = boxes + (size_t)(have ? s : 0) * O * 6;
  const float* A = angles + (size_t)(have ? s : 0) * O;
  float* GB = grad_boxes + (size_t)(have ? s : 0) * O * 6;
  float* GA = grad_angles + (size_t)(have ? s : 0) * O;
  const int cap = lpb == 1 ? OV_CAP : G;                // LDS rows of this group: [slot * G, slot * G + cap)
  const int base = slot * (lpb == 1 ? 0 : G);
  float (*my)[10] = sc + base;
  double* my_v = row_v + base;
  int* my_rr = sh_rr + base;
  int t0 = 0;
  for (int tile = 0; t0 < O; ++tile) {                  // (t0 is uniform over the grid: it depends on the tables only)
    // rows [t0, tend): the whole rooms that fit into [t0, t0 + cap), closed at the first room boundary at or behind tile_rows rows
    if (lane == 0) tile_end[slot] = min(t0 + cap, O);
    __syncthreads();
    for (int j = t0 + lane; j < min(t0 + cap, O); j += G) {
      const int rr = room_row_of(room_of_row, j, O);
      if (rr < 0 || rr >= t0 + cap) atomicMin(&tile_end[slot], j);
      else if (rr == j && j + 1 >= t0 + tile_rows) atomicMin(&tile_end[slot], j + 1);
    }
    __syncthreads();
    const int tend = tile_end[slot];
    __syncthreads();                                    // (read by every lane before lane 0 arms the next tile's)
    if (tend <= t0) break;                              // a room of more than OV_CAP rows (or a broken table): below.  (uniform)
    if (tile % (int)gridDim.y != (int)blockIdx.y) { t0 = tend; continue; }               // another workgroup's tile.  (uniform)
    for (int j = t0 + lane; j < tend; j += G) {
      const int rr = room_row_of(room_of_row, j, O);
      const Cuboid c = make_cuboid(L + (size_t)j * 6, L + (size_t)rr * 6 + 3, A[j]);
#pragma unroll
      for (int k = 0; k < 4; ++k) { my[j - t0][2 * k] = c.c[k].x; my[j - t0][2 * k + 1] = c.c[k].y; }
      my[j - t0][8] = c.h0; my[j - t0][9] = c.h1;
      my_rr[j - t0] = rr;
    }
    __syncthreads();
    for (int i0 = t0; i0 < tend; i0 += rows_per_pass) {  // (every lane of a wavefront takes every pass: the butterfly below needs them all)
      const int i = i0 + row_slot;
      const bool active = have && i < tend;
      const int rr = active ? my_rr[i - t0] : 0;
      float gx[4] = {0.f, 0.f, 0.f, 0.f}, gy[4] = {0.f, 0.f, 0.f, 0.f}, gh0 = 0.f, gh1 = 0.f;
      double acc = 0.0;
      const bool part = active && collide[i] != 0;
      if (part) {
        Cuboid a;
#pragma unroll
        for (int k = 0; k < 4; ++k) a.c[k] = make_float2(my[i - t0][2 * k], my[i - t0][2 * k + 1]);
        a.h0 = my[i - t0][8]; a.h1 = my[i - t0][9];
        int first = i;
        while (first > t0 && my_rr[first - 1 - t0] == rr) --first;
        for (int j = first + sub; j <= rr; j += OV_SUB) {
          if (j == i || !collide[j]) continue;
          const float bh0 = my[j - t0][8], bh1 = my[j - t0][9];
          const float hov = fminf(a.h1, bh1) - fmaxf(a.h0, bh0);
          if (!(hov > 0.f)) continue;                   // the pair's volume is area * max(0, hov) = 0, and so is its gradient
          float2 b[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) b[k] = make_float2(my[j - t0][2 * k], my[j - t0][2 * k + 1]);
          const float area = quad_intersection_area(a.c, b);
          if (j > i) acc += (double)(area * fmaxf(0.f, hov));                         // cuboid_pair's inter_vol
          // heights: d max(0, min(h1a, h1b) - max(h0a, h0b)); an exact tie gives each row one half (torch.minimum / torch.maximum)
          gh1 += area * (a.h1 < bh1 ? 1.f : a.h1 == bh1 ? 0.5f : 0.f);
          gh0 -= area * (a.h0 > bh0 ? 1.f : a.h0 == bh0 ? 0.5f : 0.f);
          float px[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f};
          quad_area_grad(a.c, b, px, py);
#pragma unroll
          for (int k = 0; k < 4; ++k) { gx[k] += px[k] * hov; gy[k] += py[k] * hov; }
        }
      }
#pragma unroll
      for (int o = 1; o < OV_SUB; o <<= 1) {            // the row's sub-lanes: ((u0 + u1) + (u2 + u3)), whatever the partner count
#pragma unroll
        for (int k = 0; k < 4; ++k) { gx[k] += __shfl_xor(gx[k], o, 64); gy[k] += __shfl_xor(gy[k], o, 64); }
        gh0 += __shfl_xor(gh0, o, 64); gh1 += __shfl_xor(gh1, o, 64);
        acc += __shfl_xor(acc, o, 64);
      }
      if (!active || sub != 0) continue;
      my_v[i - t0] = acc;
      // vertices and heights -> box[0:6], angle through make_cuboid's expressions: vertex = R(theta) (+- half size) + centre
      float g[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (part && i != rr) {
        const float* box = L + (size_t)i * 6;
        const float* ext = L + (size_t)rr * 6 + 3;
        const float theta = -A[i] * 0.2617993877991494f, c = cosf(theta), sn = sinf(theta);
        const float hx = (box[3] * ext[0] - box[0] * ext[0]) / 2.f, hz = (box[5] * ext[2] - box[2] * ext[2]) / 2.f;
        const float xs[4] = {-hx, -hx, hx, hx}, zs[4] = {-hz, hz, hz, -hz};
        float gxs[4], gzs[4], gcx = 0.f, gcz = 0.f, gth = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          gxs[k] = c * gx[k] - sn * gy[k]; gzs[k] = sn * gx[k] + c * gy[k];
          gcx += gx[k]; gcz += gy[k];
          gth += gx[k] * (-sn * xs[k] + c * zs[k]) - gy[k] * (c * xs[k] + sn * zs[k]);
        }
        const float gmnx = gxs[0] + gxs[1], gmxx = gxs[2] + gxs[3], gmnz = gzs[0] + gzs[3], gmxz = gzs[1] + gzs[2];
        g[0] = ext[0] * ((gmnx - gmxx + gcx) / 2.f); g[3] = ext[0] * ((gmxx - gmnx + gcx) / 2.f);
        g[2] = ext[2] * ((gmnz - gmxz + gcz) / 2.f); g[5] = ext[2] * ((gmxz - gmnz + gcz) / 2.f);
        g[1] = ext[1] * gh0; g[4] = ext[1] * gh1;
        g[6] = -0.2617993877991494f * gth;
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) GB[(size_t)i * 6 + q] = accumulate ? GB[(size_t)i * 6 + q] + weight * g[q] : weight * g[q];
      GA[i] = accumulate ? GA[i] + weight * g[6] : weight * g[6];
    }
    __syncthreads();
    if (have)
    for (int i = t0 + lane; i < tend; i += G) {
      if (my_rr[i - t0] != i) continue;                 // the room row: the last row of its room, the room's one writer
      const int id = room_id[i];
      if (id < 0 || id >= n_rooms) continue;
      int first = i;
      while (first > t0 && my_rr[first - 1 - t0] == i) --first;
      double v = 0.0;
      for (int j = first; j <= i; ++j) v += my_v[j - t0];
      penalty_out[(size_t)s * n_rooms + id] = v;
    }
    __syncthreads();
    t0 = tend;
  }
  if (have && t0 < O && blockIdx.y == 0)                // what no tile could hold: NaN penalties, zero gradients
    for (int i = t0 + lane; i < O; i += G) {
      if (!accumulate) {
#pragma unroll
        for (int q = 0; q < 6; ++q) GB[(size_t)i * 6 + q] = 0.f;
        GA[i] = 0.f;
      }
      const int id = room_id[i];
      if (room_of_row[i] == i && id >= 0 && id < n_rooms) penalty_out[(size_t)s * n_rooms + id] = (double)__builtin_nanf("");
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

extern "C" int sln_layout_overlap_penalty(const float* boxes, const float* angles, const int32_t* room_of_row, const unsigned char* collide,
                                          const int32_t* room_id, int n_rooms, int S, int O, float weight, int accumulate, double* penalty_out,
                                          float* grad_boxes, float* grad_angles, void* stream) {
  if (!boxes || !angles || !room_of_row || !collide || !room_id || !penalty_out || !grad_boxes || !grad_angles) return SLN_E_BADARG;
  if (S < 0 || O < 0 || n_rooms < 1 || !(weight >= 0.f) || (accumulate != 0 && accumulate != 1)) return SLN_E_BADARG;
  if (S == 0 || O == 0) return 0;
  // OV_SUB lanes per row: a group of G = the power of two >= OV_SUB * O lanes per layout when that is at most the workgroup (several
  // layouts per workgroup), otherwise the whole workgroup in passes of G / OV_SUB rows; tiles of about PEN_TILE rows over gridDim.y
  constexpr int PEN_TILE = 48;                          // (closed at the next room boundary: 52 rows for rooms of 13, one pass of 64)
  int G = OV_BLOCK;
  if (OV_SUB * O <= OV_BLOCK) { G = 8; while (G < OV_SUB * O) G <<= 1; }
  const int lpb = OV_BLOCK / G, chunks = O / PEN_TILE < 1 ? 1 : O / PEN_TILE > 256 ? 256 : O / PEN_TILE;
  hipLaunchKernelGGL(layout_overlap_penalty_kernel, dim3(sln_cdiv(S, lpb), chunks), dim3(OV_BLOCK), 0, static_cast<hipStream_t>(stream), boxes,
                     angles, room_of_row, collide, room_id, n_rooms, S, O, G, PEN_TILE, weight, accumulate, penalty_out, grad_boxes, grad_angles);
  SLN_CHECK_LAUNCH();
  return 0;
}
