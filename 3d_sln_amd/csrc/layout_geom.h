// The cuboid of one layout row as the reference forms it (testing/test_render_refine.py:90-110 get_boxes, testing/test_plot2d.py:88-110
// plot2d, testing/test_utils.py:7-40 get_eight_coors_bbox_new), shared by layout_iou.hip and layout_plot.hip.  float32 throughout;
// the units that include this are compiled with contraction off (build.py).
#ifndef SLN_LAYOUT_GEOM_H
#define SLN_LAYOUT_GEOM_H
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float shoelace4(const float2 q[4]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const float2 a = q[k], b = q[(k + 1) & 3]; s += a.x * b.y - b.x * a.y; }
  return 0.5f * s;
}

struct Cuboid { float2 c[4]; float h0, h1; };

// get_boxes (:90-110) + get_eight_coors_bbox_new of one row: `box` [6], `ext` = the room row's box[3:6]
__device__ __forceinline__ Cuboid make_cuboid(const float* __restrict__ box, const float* __restrict__ ext, const float angle) {
  float mn[3], mx[3], ctr[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    mn[q] = box[q] * ext[q]; mx[q] = box[3 + q] * ext[q];
    ctr[q] = (mx[q] + mn[q]) / 2.f;
    mn[q] -= ctr[q]; mx[q] -= ctr[q];
  }
  const float theta = -angle * 0.2617993877991494f;                // float32(2 pi / 24), as torch multiplies a float tensor by a python scalar
  const float c = cosf(theta), s = sinf(theta);
  Cuboid r;
  const float xs[4] = {mn[0], mn[0], mx[0], mx[0]}, zs[4] = {mn[2], mx[2], mx[2], mn[2]}, ys[4] = {mn[1], mn[1], mx[1], mn[1]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    r.c[k].x = ((c * xs[k] + 0.f * ys[k]) + s * zs[k]) + ctr[0];
    r.c[k].y = ((-s * xs[k] + 0.f * ys[k]) + c * zs[k]) + ctr[2];
  }
  r.h0 = mn[1] + ctr[1]; r.h1 = mx[1] + ctr[1];
  return r;
}

// a row's room row, or -1 when the table entry is no row at or behind it
__device__ __forceinline__ int room_row_of(const int* __restrict__ room_of_row, int i, int O) {
  const int r = room_of_row[i];
  return (r >= i && r < O) ? r : -1;
}

}  // namespace
#endif  // SLN_LAYOUT_GEOM_H
