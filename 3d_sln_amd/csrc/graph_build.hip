// Scene-graph builder on the device: the work of SuncgDataset.__getitem__ + suncg_collate_fn
// (reference data/suncg_dataset.py:110-353, utils.py:36-80 compute_rel) for a whole batch of rooms.
//
// The room table (classes, raw boxes, rotations, room boxes, size thresholds) stays resident in HBM; a batch is a
// list of room indices plus the random decisions the reference draws from python's `random` (which partner, subject /
// object order, which size attribute) - injected, so that the result is bit-identical to the reference given the same
// draws.  One wavefront per room:
//   plan : number of rows / triples of every room ('on' pairs depend on the geometry) + exclusive scan
//   emit : objs, boxes (room-normalised), angles, attributes, triples (reference order: 'on' pairs by (cur, other),
//          one drawn pair per object, then the __in_room__ rows), obj_to_img, triple_to_img.
// compute_rel is evaluated in float32 exactly as the reference does (left-to-right, no contraction: this file is
// built with -ffp-contract=off); its atan2 sector test is replaced by the equivalent comparisons
// (oracle/graph_build_ref.py::sector_by_compare, tests/test_oracle_graph_build.py).
#include "sln_common.h"
#include "../../include/sln_hip.h"

namespace {

enum { P_IN_ROOM = 0, P_LEFT = 1, P_RIGHT = 2, P_BEHIND = 3, P_FRONT = 4, P_INSIDE = 5, P_SURROUND = 6, P_LEFT_T = 7,
       P_RIGHT_T = 8, P_FRONT_T = 9, P_BEHIND_T = 10, P_ON = 15 };

struct Box { float x0, y0, z0, x1, y1, z1; };

__device__ __forceinline__ Box load_box(const float* p) { Box b; b.x0 = p[0]; b.y0 = p[1]; b.z0 = p[2]; b.x1 = p[3]; b.y1 = p[4]; b.z1 = p[5]; return b; }

__device__ __forceinline__ bool rel_is_on(const Box& s, const Box& o) {   // utils.py:45-52
  const float c1x = (s.x0 + s.x1) / 2.f, c1y = (s.y0 + s.y1) / 2.f, c1z = (s.z0 + s.z1) / 2.f;
  const float c2y = (o.y0 + o.y1) / 2.f;
  if (c1x >= o.x0 && c1x <= o.x1 && c1z >= o.z0 && c1z <= o.z1) {
    const float delta1 = c1y - c2y;
    const float delta2 = (s.y1 - s.y0 + o.y1 - o.y0) / 2.f;
    return fabsf(delta1 - delta2) < 0.05f;
  }
  return false;
}

__device__ __forceinline__ int compute_rel(const Box& s, const Box& o) {  // utils.py:36-80
  if (rel_is_on(s, o)) return P_ON;
  const float dx = (s.x0 + s.x1) / 2.f - (o.x0 + o.x1) / 2.f;
  const float dz = (s.z0 + s.z1) / 2.f - (o.z0 + o.z1) / 2.f;
  const float area_s = (s.x1 - s.x0) * (s.z1 - s.z0);
  const float area_o = (o.x1 - o.x0) * (o.z1 - o.z0);
  const float ix0 = fmaxf(s.x0, o.x0), ix1 = fminf(s.x1, o.x1);
  const float iz0 = fmaxf(s.z0, o.z0), iz1 = fminf(s.z1, o.z1);
  const float area_i = fmaxf(0.f, ix1 - ix0) * fmaxf(0.f, iz1 - iz0);
  const float iou = area_i / (area_s + area_o - area_i);
  const bool touching = 0.0001f < iou && iou < 0.5f;
  if (s.x0 < o.x0 && s.x1 > o.x1 && s.z0 < o.z0 && s.z1 > o.z1) return P_SURROUND;
  if (s.x0 > o.x0 && s.x1 < o.x1 && s.z0 > o.z0 && s.z1 < o.z1) return P_INSIDE;
  if (dx < 0.f && fabsf(dz) <= -dx) return touching ? P_RIGHT_T : P_LEFT;        // theta >= 3pi/4 or <= -3pi/4
  if (dz < 0.f && fabsf(dx) < -dz) return touching ? P_BEHIND_T : P_BEHIND;      // -3pi/4 <= theta < -pi/4
  if ((dx > 0.f && -dx <= dz && dz < dx) || (dx == 0.f && dz == 0.f)) return touching ? P_LEFT_T : P_RIGHT;
  return touching ? P_FRONT_T : P_FRONT;
}

__device__ __forceinline__ int lane_prefix(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// number of 'on' pairs of one room, counted by the whole wavefront (uniform result)
__device__ int count_on_pairs(const float* bbox, int n, int lane) {
  int total = 0;
  for (int cur = 0; cur < n; ++cur) {
    const Box s = load_box(bbox + (size_t)cur * 6);
    for (int o0 = 0; o0 < n; o0 += 64) {
      const int oth = o0 + lane;
      bool hit = false;
      if (oth < n && oth != cur) hit = rel_is_on(s, load_box(bbox + (size_t)oth * 6));
      total += __popcll(__ballot(hit));
    }
  }
  return total;
}

__global__ __launch_bounds__(64) void graph_count_kernel(SlnRoomTable tab, const int* __restrict__ room_idx, int B, int* __restrict__ counts) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int r = room_idx[b];
  const bool valid = r >= 0 && r < tab.n_rooms;
  r = valid ? r : 0;
  const int first = tab.room_off[r], n = tab.room_off[r + 1] - first;
  const int n_on = count_on_pairs(tab.bbox + (size_t)first * 6, n, lane);
  if (lane == 0) {
    counts[2 * b + 0] = valid ? n + 1 : -1;                 // rows: objects + the room (negative: bad room index)
    counts[2 * b + 1] = n_on + (n >= 2 ? n : 0) + n;        // 'on' pairs + one drawn pair per object + __in_room__
  }
}

// exclusive scan of the per-room counts: off[0..B] rows, off[B+1 .. 2B+1] triples, off[2B+2] = number of bad room indices
__global__ __launch_bounds__(256) void graph_scan_kernel(const int* __restrict__ counts, int B, int* __restrict__ off) {
  __shared__ int part[2][256];
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  const int per = (B + 255) / 256, lo = min(B, tid * per), hi = min(B, lo + per);
  if (tid == 0) bad_s = 0;
  __syncthreads();
  int s0 = 0, s1 = 0, bad = 0;
  for (int i = lo; i < hi; ++i) { const int c = counts[2 * i]; bad += c < 0; s0 += max(c, 0); s1 += counts[2 * i + 1]; }
  part[0][tid] = s0; part[1][tid] = s1;
  if (bad) atomicAdd(&bad_s, bad);
  __syncthreads();
  if (tid == 0) {
    int a = 0, c = 0;
    for (int i = 0; i < 256; ++i) { const int t0 = part[0][i], t1 = part[1][i]; part[0][i] = a; part[1][i] = c; a += t0; c += t1; }
    off[B] = a; off[2 * B + 1] = c; off[2 * B + 2] = bad_s;
  }
  __syncthreads();
  int a = part[0][tid], c = part[1][tid];
  for (int i = lo; i < hi; ++i) { off[i] = a; off[B + 1 + i] = c; a += max(counts[2 * i], 0); c += counts[2 * i + 1]; }
}

__global__ __launch_bounds__(64) void graph_emit_kernel(SlnRoomTable tab, const int* __restrict__ room_idx, int B,
                                                        const int* __restrict__ off, SlnGraphDraws draws, SlnGraphBatch out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int r = room_idx[b];
  if (r < 0 || r >= tab.n_rooms) return;
  const int first = tab.room_off[r], n = tab.room_off[r + 1] - first;
  const int row0 = off[b], trip0 = off[B + 1 + b];
  const int draw0 = row0 - b;                                  // draws hold one entry per NON-room row, in batch order
  const float* bbox = tab.bbox + (size_t)first * 6;
  const float rx = tab.room_bbox[3 * r + 0], ry = tab.room_bbox[3 * r + 1], rz = tab.room_bbox[3 * r + 2];
  if (lane == 0 && out.ids) out.ids[b] = tab.room_id ? tab.room_id[r] : r;

  // ---- rows: objs, boxes (normalised after the triples in the reference, independent here), angles, attributes ----
  for (int i = lane; i <= n; i += 64) {
    const size_t row = (size_t)row0 + i;
    float* bo = out.boxes + row * 6;
    int attr = 0;
    if (i < n) {
      const Box s = load_box(bbox + (size_t)i * 6);
      const float x0 = s.x0 / rx, y0 = s.y0 / ry, z0 = s.z0 / rz, x1 = s.x1 / rx, y1 = s.y1 / ry, z1 = s.z1 / rz;
      bo[0] = x0; bo[1] = y0; bo[2] = z0; bo[3] = x1; bo[4] = y1; bo[5] = z1;
      const int cls = tab.cls[first + i];
      const int mode = draws.attr_mode[draw0 + i];               // 0 none, 1 height test, 2 volume test
      const bool known = cls >= 0 && cls < tab.n_classes && tab.has_size[cls];
      if (mode != 0 && known) {
        const float* th = tab.size_thr + 4 * cls;
        const float height = y1 - y0;
        const float volume = (x1 - x0) * (y1 - y0) * (z1 - z0);
        if (!tab.use_attr_30) {
          if (mode == 1) attr = height > th[0] ? 1 : 2;          // tall / short
          else attr = volume > th[1] ? 3 : 4;                    // large / small
        } else {
          if (mode == 1) attr = height > th[0] ? 1 : (height < th[1] ? 2 : 0);
          else attr = volume > th[2] ? 3 : (volume < th[3] ? 4 : 0);
        }
      }
      out.objs[row] = cls; out.angles[row] = tab.rot[first + i];
    } else {
      bo[0] = 0.f; bo[1] = 0.f; bo[2] = 0.f; bo[3] = rx; bo[4] = ry; bo[5] = rz;
      out.objs[row] = 0; out.angles[row] = 0;                    // '__room__' (vocab index 0), angle 0
    }
    out.attributes[row] = attr;
    out.obj_to_img[row] = b;
  }

  // ---- triples ----
  int t = trip0;
  for (int cur = 0; cur < n; ++cur) {                            // 'on' pairs, (cur, other) order kept by the compaction
    const Box s = load_box(bbox + (size_t)cur * 6);
    for (int o0 = 0; o0 < n; o0 += 64) {
      const int oth = o0 + lane;
      bool hit = false;
      if (oth < n && oth != cur) hit = rel_is_on(s, load_box(bbox + (size_t)oth * 6));
      const unsigned long long m = __ballot(hit);
      if (hit) {
        int64_t* tr = out.triples + (size_t)(t + lane_prefix(m, lane)) * 3;
        tr[0] = row0 + cur; tr[1] = P_ON; tr[2] = row0 + oth;
      }
      t += __popcll(m);
    }
  }
  if (n >= 2) {
    for (int cur = lane; cur < n; cur += 64) {                   // one drawn pair per object (suncg_dataset.py:189-205)
      int oth = draws.other[draw0 + cur];
      oth = min(max(oth, 0), n - 1);
      const bool keep = draws.swap[draw0 + cur] != 0;
      const int s = keep ? cur : oth, o = keep ? oth : cur;
      const int p = compute_rel(load_box(bbox + (size_t)s * 6), load_box(bbox + (size_t)o * 6));
      int64_t* tr = out.triples + (size_t)(t + cur) * 3;
      tr[0] = row0 + s; tr[1] = p; tr[2] = row0 + o;
    }
    t += n;
  }
  for (int i = lane; i < n; i += 64) {
    int64_t* tr = out.triples + (size_t)(t + i) * 3;
    tr[0] = row0 + i; tr[1] = P_IN_ROOM; tr[2] = row0 + n;
  }
  t += n;
  for (int i = trip0 + lane; i < t; i += 64) out.triple_to_img[i] = b;
}

// The random decisions of a batch drawn on the device in ONE launch (round 3; host/suncg_dataset.py::device_draws used to spell
// them as ~15 ATen launches): Philox-4x32-10 keyed by two 64-bit words in device memory (the caller takes them from its torch
// generator, so the generator's stream advances and nothing is read back), counter = the object's row among the non-room rows
// of the batch; the four words of a counter are the four uniforms of one object (suncg_dataset.py:189-196, 236-282):
//   other = uniform choice among the n - 1 other objects, swap = u > 0.5, attribute mode = none / height / volume.
__device__ __forceinline__ void gb_philox(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned int)p1;
    const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned int)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

__global__ __launch_bounds__(64) void graph_draw_kernel(SlnRoomTable tab, const int* __restrict__ room_idx, int B,
                                                        const int* __restrict__ off, const long long* __restrict__ key,
                                                        int* __restrict__ other, unsigned char* __restrict__ swap,
                                                        unsigned char* __restrict__ mode) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int r = room_idx[b];
  if (r < 0 || r >= tab.n_rooms) return;
  const int first = tab.room_off[r], n = tab.room_off[r + 1] - first;
  const int base = off[b] - b;                       // rows of earlier rooms minus their room rows = first draw slot of this room
  const unsigned long long k0 = (unsigned long long)key[0], k1 = (unsigned long long)key[1];
  for (int cur = lane; cur < n; cur += 64) {
    const unsigned int j = (unsigned int)(base + cur);
    unsigned int c[4] = {j, (unsigned int)(k1 >> 32), (unsigned int)k1, 0x5ce9e6a1u};
    gb_philox(c, (unsigned int)k0, (unsigned int)(k0 >> 32));
    const float u0 = (float)(c[0] >> 8) * 5.9604644775390625e-08f, u1 = (float)(c[1] >> 8) * 5.9604644775390625e-08f;   // [0, 1)
    const float u2 = (float)(c[2] >> 8) * 5.9604644775390625e-08f, u3 = (float)(c[3] >> 8) * 5.9604644775390625e-08f;
    int k = min((int)(u0 * (float)(n - 1)), n - 2);
    k = max(k, 0);
    other[j] = k + (k >= cur ? 1 : 0);
    swap[j] = u1 > 0.5f ? 1 : 0;
    const bool known = tab.has_size[tab.cls[first + cur]] != 0;
    mode[j] = (u2 > 0.5f || !known) ? 0 : (u3 > 0.5f ? 1 : 2);
  }
}

// ---- evaluation of layouts (reference testing/test_acc_mean_std.py:10-125, testing/test_utils.py:93-152) ----------------------------
struct PredTable { int t[16]; };          // compute_rel's relation order -> the vocabulary's predicate index (-1: name not in the vocabulary)

// restore_box (test_utils.py:119-132) for one row, without touching the caller's tensor: a non-room row is scaled by the first room
// row at or after it (x by its [3], y by [4], z by [5], float32); room rows and rows behind the last room row keep their values.
__device__ __forceinline__ Box restored_row(const float* L, const int64_t* __restrict__ objs, int O, int i, int room_cls) {
  Box b = load_box(L + (size_t)i * 6);
  if (objs[i] == room_cls) return b;
  int j = i + 1;
  while (j < O && objs[j] != room_cls) ++j;
  if (j < O) {
    const float* r = L + (size_t)j * 6;
    const float sx = r[3], sy = r[4], sz = r[5];
    b.x0 *= sx; b.x1 *= sx; b.y0 *= sy; b.y1 *= sy; b.z0 *= sz; b.z1 *= sz;
  }
  return b;
}

// scene_graph_acc (test_utils.py:135-152) for S layouts at once: grid (triple blocks, S), one triple per thread.  rel = 16: compute_rel
// returned None (a NaN centre difference makes atan2 NaN and no sector matches; the builder's compute_rel falls through to 'front').
__global__ __launch_bounds__(256) void layout_rel_kernel(const float* __restrict__ boxes, int O, const int64_t* __restrict__ objs,
                                                         const int64_t* __restrict__ triples, int T, int room_cls, PredTable tab,
                                                         unsigned long long* __restrict__ good, unsigned long long* __restrict__ conf) {
  const int s = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  bool hit = false;
  if (t < T) {
    const int64_t a = triples[3 * (size_t)t], pg = triples[3 * (size_t)t + 1], b = triples[3 * (size_t)t + 2];
    if (a >= 0 && a < O && b >= 0 && b < O) {
      const float* L = boxes + (size_t)s * O * 6;
      int rel;
      if (objs[b] == room_cls) {
        rel = P_IN_ROOM;                                         // utils.py:41-42, before any geometry
      } else {
        const Box bs = restored_row(L, objs, O, (int)a, room_cls), bo = restored_row(L, objs, O, (int)b, room_cls);
        rel = compute_rel(bs, bo);
        const float dx = (bs.x0 + bs.x1) / 2.f - (bo.x0 + bo.x1) / 2.f, dz = (bs.z0 + bs.z1) / 2.f - (bo.z0 + bo.z1) / 2.f;
        if (rel != P_ON && rel != P_SURROUND && rel != P_INSIDE && (__builtin_isnan(dx) || __builtin_isnan(dz))) rel = 16;
      }
      hit = rel < 16 && tab.t[rel] >= 0 && (int64_t)tab.t[rel] == pg;
      if (conf) {
        int row = -1;
        for (int r = 0; r < 16; ++r) row = (row < 0 && tab.t[r] >= 0 && (int64_t)tab.t[r] == pg) ? r : row;
        if (row >= 0) atomicAdd(conf + ((size_t)s * 16 + row) * 17 + rel, 1ull);
      }
    }
  }
  const unsigned long long m = __ballot(hit);                    // integer counts: one atomic per wavefront, order-independent
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(good + s, (unsigned long long)__popcll(m));
}

// fixed-order block sum of NV fp64 values (blockDim.x = NT): the same tree every launch
template <int NV, int NT>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*sh)[NT]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; ++k) sh[k][tid] = v[k];
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < NV; ++k) sh[k][tid] += sh[k][tid + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = sh[k][0];
}

// get_std (test_acc_mean_std.py:39-69) of one batch: per element (angle bin, position x/y/z, size x/y/z of every row) the population
// std over the S samples, two-pass in fp64; then the mean over the elements of each kind.  One workgroup: fixed element-to-thread
// assignment and a fixed reduction tree, so the figures are bit-identical run to run.  out[0..2] += (angle, position, size).
// 1024 threads: the per-element passes are a chain of dependent loads (latency-bound); 256 threads took 71 us at O = 640, S = 10.
__global__ __launch_bounds__(1024) void layout_spread_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ bins, int S, int O,
                                                            double* __restrict__ out) {
  __shared__ double sh[3][1024];
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t so = (size_t)O * 6;
  for (int e = threadIdx.x; e < 7 * O; e += 1024) {
    int kind, r, c;
    if (e < O) { kind = 0; r = e; c = 0; }
    else { const int e2 = e - O; kind = 1 + e2 / (3 * O); r = (e2 % (3 * O)) / 3; c = e2 % 3; }
    double sum = 0.0;
    for (int k = 0; k < S; ++k) {
      const float* p = boxes + k * so + (size_t)r * 6 + c;
      const double v = kind == 0 ? (double)bins[(size_t)k * O + r] : kind == 1 ? (double)(p[0] / 2.f + p[3] / 2.f) : (double)fabsf(p[0] - p[3]);
      sum += v;
    }
    const double mean = sum / S;
    double ss = 0.0;
    for (int k = 0; k < S; ++k) {
      const float* p = boxes + k * so + (size_t)r * 6 + c;
      const double v = kind == 0 ? (double)bins[(size_t)k * O + r] : kind == 1 ? (double)(p[0] / 2.f + p[3] / 2.f) : (double)fabsf(p[0] - p[3]);
      ss += (v - mean) * (v - mean);
    }
    acc[kind] += sqrt(ss / S);
  }
  block_sum<3, 1024>(acc, sh);
  if (threadIdx.x == 0) {
    out[0] += acc[0] / O;
    out[1] += acc[1] / (3.0 * O);
    out[2] += acc[2] / (3.0 * O);
  }
}

// F.l1_loss(layout, gt) of each of S layouts (test_acc_mean_std.py:111-113): fp64 sum of the float32 |a - b|, fixed tree; out[s] += mean
__global__ __launch_bounds__(256) void layout_l1_kernel(const float* __restrict__ boxes, const float* __restrict__ gt, int O, double* __restrict__ out) {
  __shared__ double sh[1][256];
  const int s = blockIdx.x;
  const size_t n = (size_t)O * 6;
  const float* L = boxes + s * n;
  double acc[1] = {0.0};
  for (size_t i = threadIdx.x; i < n; i += 256) acc[0] += (double)fabsf(L[i] - gt[i]);
  block_sum<1, 256>(acc, sh);
  if (threadIdx.x == 0) out[s] += acc[0] / (double)n;
}

// The two baselines of get_acc_l1 (test_acc_mean_std.py:108-110): out[0] = random_scene (test_utils.py:93-116: room rows copied, every
// other row re-centred at a uniform (x, y, z) with its own extent), out[1] = boxes + float32(hstack([off, off])), off ~ N(0, 0.1).
// Draws: injected (uni / nrm [O, 3]; only the non-room rows of uni are read) or, with key != NULL, Philox keyed by key[0..1] in device
// memory, one counter per row.
__global__ __launch_bounds__(64) void layout_baselines_kernel(const float* __restrict__ gt, const int64_t* __restrict__ objs, int O, int room_cls,
                                                              const float* __restrict__ uni, const float* __restrict__ nrm,
                                                              const long long* __restrict__ key, float* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= O) return;
  float u[3], n[3];
  if (key) {
    const unsigned long long k0 = (unsigned long long)key[0], k1 = (unsigned long long)key[1];
    unsigned int c[4] = {(unsigned int)i, (unsigned int)(k1 >> 32), (unsigned int)k1, 0x3c6ef372u};
    gb_philox(c, (unsigned int)k0, (unsigned int)(k0 >> 32));
    unsigned int d[4] = {(unsigned int)i, (unsigned int)(k1 >> 32), (unsigned int)k1, 0xa54ff53au};
    gb_philox(d, (unsigned int)k0, (unsigned int)(k0 >> 32));
    for (int q = 0; q < 3; ++q) u[q] = (float)(c[q] >> 8) * 5.9604644775390625e-08f;                      // [0, 1)
    // Box-Muller on (0, 1] x [0, 1): two normal pairs, three used
    const float r0 = sqrtf(-2.f * logf((float)((d[0] >> 8) + 1u) * 5.9604644775390625e-08f));
    const float r1 = sqrtf(-2.f * logf((float)((d[2] >> 8) + 1u) * 5.9604644775390625e-08f));
    const float a0 = 6.2831853071795865f * ((float)(d[1] >> 8) * 5.9604644775390625e-08f);
    const float a1 = 6.2831853071795865f * ((float)(d[3] >> 8) * 5.9604644775390625e-08f);
    n[0] = 0.1f * (r0 * cosf(a0)); n[1] = 0.1f * (r0 * sinf(a0)); n[2] = 0.1f * (r1 * cosf(a1));
  } else {
    for (int q = 0; q < 3; ++q) { u[q] = uni[(size_t)i * 3 + q]; n[q] = nrm[(size_t)i * 3 + q]; }
  }
  const float* g = gt + (size_t)i * 6;
  float* rnd = out + (size_t)i * 6;
  float* per = out + ((size_t)O + i) * 6;
  const bool room = objs[i] == room_cls;
  for (int q = 0; q < 3; ++q) {
    const float h = (g[q + 3] - g[q]) / 2.f;
    rnd[q] = room ? g[q] : u[q] - h;
    rnd[q + 3] = room ? g[q + 3] : u[q] + h;
    per[q] = g[q] + n[q];
    per[q + 3] = g[q + 3] + n[q];
  }
}

}  // namespace

extern "C" int sln_graph_draw(const SlnRoomTable* tab, const int* room_idx, int B, const int* offsets, const int64_t* key,
                              int* other, unsigned char* swap, unsigned char* attr_mode, void* stream) {
  if (!tab || !room_idx || !offsets || !key || !other || !swap || !attr_mode || B < 0) return -1;
  if (B == 0) return 0;
  hipLaunchKernelGGL(graph_draw_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), *tab, room_idx, B, offsets,
                     reinterpret_cast<const long long*>(key), other, swap, attr_mode);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_graph_plan(const SlnRoomTable* tab, const int* room_idx, int B, int* counts, int* offsets, void* stream) {
  if (!tab || !room_idx || !counts || !offsets || B < 0) return -1;
  if (B == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(graph_count_kernel, dim3(B), dim3(64), 0, st, *tab, room_idx, B, counts);
  SLN_CHECK_LAUNCH();
  hipLaunchKernelGGL(graph_scan_kernel, dim3(1), dim3(256), 0, st, counts, B, offsets);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_graph_emit(const SlnRoomTable* tab, const int* room_idx, int B, const int* offsets, const SlnGraphDraws* draws,
                              const SlnGraphBatch* out, void* stream) {
  if (!tab || !room_idx || !offsets || !draws || !out || B < 0) return -1;
  if (!out->objs || !out->boxes || !out->triples || !out->angles || !out->attributes || !out->obj_to_img || !out->triple_to_img) return -1;
  if (!draws->other || !draws->swap || !draws->attr_mode) return -1;
  if (B == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(graph_emit_kernel, dim3(B), dim3(64), 0, st, *tab, room_idx, B, offsets, *draws, *out);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_layout_relation_acc(const float* boxes, int S, int O, int box_dim, const int64_t* objs, const int64_t* triples, int T, int room_cls,
                                       const int* pred_table_host, int64_t* good, int64_t* confusion, void* stream) {
  if (!boxes || !objs || !pred_table_host || !good || S < 0 || O < 0 || T < 0 || box_dim != 6 || (T > 0 && !triples)) return -1;
  if (S == 0 || T == 0 || O == 0) return 0;
  if (S > 65535) return -1;
  PredTable tab;
  for (int r = 0; r < 16; ++r) tab.t[r] = pred_table_host[r];
  hipLaunchKernelGGL(layout_rel_kernel, dim3((T + 255) / 256, S), dim3(256), 0, static_cast<hipStream_t>(stream), boxes, O, objs, triples, T,
                     room_cls, tab, reinterpret_cast<unsigned long long*>(good), reinterpret_cast<unsigned long long*>(confusion));
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_layout_spread(const float* boxes, const int64_t* angle_bins, int S, int O, int box_dim, double* out, void* stream) {
  if (!boxes || !angle_bins || !out || S < 1 || O < 0 || box_dim != 6 || O > (1 << 27)) return -1;
  if (O == 0) return 0;
  hipLaunchKernelGGL(layout_spread_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), boxes, angle_bins, S, O, out);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_layout_l1(const float* boxes, int S, int O, int box_dim, const float* gt, double* out, void* stream) {
  if (!boxes || !gt || !out || S < 0 || O < 0 || box_dim != 6) return -1;
  if (S == 0 || O == 0) return 0;
  hipLaunchKernelGGL(layout_l1_kernel, dim3(S), dim3(256), 0, static_cast<hipStream_t>(stream), boxes, gt, O, out);
  SLN_CHECK_LAUNCH();
  return 0;
}

extern "C" int sln_layout_baselines(const float* gt, const int64_t* objs, int O, int box_dim, int room_cls, const float* uniforms,
                                    const float* normals, const int64_t* key, float* out, void* stream) {
  if (!gt || !objs || !out || O < 0 || box_dim != 6) return -1;
  if (!key && (!uniforms || !normals)) return -1;
  if (O == 0) return 0;
  hipLaunchKernelGGL(layout_baselines_kernel, dim3((O + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), gt, objs, O, room_cls,
                     uniforms, normals, reinterpret_cast<const long long*>(key), out);
  SLN_CHECK_LAUNCH();
  return 0;
}
