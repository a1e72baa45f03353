// The argument checks of the observed-frame entry points - sln_observed_target, sln_observed_prefilter, sln_reproject_faces,
// sln_reproject_compose, sln_reproject_fuse - run from a program of their own so that the host code can be built with a sanitizer
// (never load a sanitized library into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude -I3d_sln_amd/csrc \
//         tools/observed_args_check.cpp 3d_sln_amd/csrc/observed_target.hip 3d_sln_amd/csrc/observed_prefilter.hip \
//         3d_sln_amd/csrc/observed_reproject.hip 3d_sln_amd/csrc/observed_fuse.hip -o observed_args_check && ./observed_args_check
//
// Every call below must be refused before anything is launched: the "device" pointers are small host arrays that a correct check never
// dereferences, the host tables are sized exactly NC entries, so a read past a table is the sanitizer's to report.  Each case changes ONE
// argument of a call that is otherwise sound, and the expected codes are those include/sln_hip.h states.  Needs no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sln_hip.h"

static int failures = 0;

static void expect(const char* what, int rc, int want) {
  if (rc != want) { std::printf("FAIL %s: returned %d, expected %d\n", what, rc, want); ++failures; }
  else std::printf("ok   %s\n", what);
}

template <typename T>
static T* off(T* p, int bytes) { return reinterpret_cast<T*>(reinterpret_cast<char*>(p) + bytes); }

alignas(16) static float depth[64], out[64], wgt[64], kk[64], pose[64], K[64];
alignas(16) static unsigned char labels[64], lout[64], u8a[64], u8b[64], u8c[64];
alignas(16) static int32_t ws[64], status[4], fi[64];
alignas(16) static int64_t hits[8], wins[8], counts[8];
static const int U = SLN_E_UNSUPPORTED, A = SLN_E_BADARG;
static const float NaN = std::nanf("");

static void target_checks() {
  const int NC = 32, NCH = 70, B = 2, S = 8;
  std::vector<int32_t> chan(NC), dch(NC);
  for (int c = 0; c < NC; ++c) { chan[c] = c; dch[c] = c < 3 ? -1 : c - 3; }
  auto call = [&](const float* d, const unsigned char* l, int b, int s, int nc, const int32_t* ch, const int32_t* dc, int nch, void* w, float* o,
                  int32_t* st) { return sln_observed_target(d, l, b, s, nc, ch, dc, nch, w, o, st, nullptr); };

  expect("S = 6", call(depth, labels, B, 6, NC, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("S = 0", call(depth, labels, B, 0, NC, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("S = 4100", call(depth, labels, B, 4100, NC, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("B = 0", call(depth, labels, 0, S, NC, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("B = 65536", call(depth, labels, 65536, S, NC, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("NC = 0", call(depth, labels, B, S, 0, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("NC = 65 (the tables hold 32: nothing past them may be read)", call(depth, labels, B, S, 65, chan.data(), dch.data(), NCH, ws, out, status), U);
  expect("nch = 69", call(depth, labels, B, S, NC, chan.data(), dch.data(), 69, ws, out, status), U);
  expect("nch = 73", call(depth, labels, B, S, NC, chan.data(), dch.data(), 73, ws, out, status), U);
  expect("nch = 40", call(depth, labels, B, S, NC, chan.data(), dch.data(), 40, ws, out, status), U);
  { auto d = dch; d[31] = -1; expect("28 owned channels under nch = 70", call(depth, labels, B, S, NC, chan.data(), d.data(), NCH, ws, out, status), U); }

  expect("null depth", call(nullptr, labels, B, S, NC, chan.data(), dch.data(), NCH, ws, out, status), A);
  expect("null labels", call(depth, nullptr, B, S, NC, chan.data(), dch.data(), NCH, ws, out, status), A);
  expect("null chan", call(depth, labels, B, S, NC, nullptr, dch.data(), NCH, ws, out, status), A);
  expect("null dch", call(depth, labels, B, S, NC, chan.data(), nullptr, NCH, ws, out, status), A);
  expect("null workspace", call(depth, labels, B, S, NC, chan.data(), dch.data(), NCH, nullptr, out, status), A);
  expect("null out", call(depth, labels, B, S, NC, chan.data(), dch.data(), NCH, ws, nullptr, status), A);
  expect("null status", call(depth, labels, B, S, NC, chan.data(), dch.data(), NCH, ws, out, nullptr), A);
  expect("depth 4 bytes off", call(depth + 1, labels, B, S, NC, chan.data(), dch.data(), NCH, ws, out, status), A);
  expect("out 8 bytes off", call(depth, labels, B, S, NC, chan.data(), dch.data(), NCH, ws, out + 2, status), A);
  expect("labels 1 byte off", call(depth, labels + 1, B, S, NC, chan.data(), dch.data(), NCH, ws, out, status), A);
  expect("workspace 2 bytes off", call(depth, labels, B, S, NC, chan.data(), dch.data(), NCH, reinterpret_cast<char*>(ws) + 2, out, status), A);
  { auto c = chan; c[0] = 40; expect("chan = 40", call(depth, labels, B, S, NC, c.data(), dch.data(), NCH, ws, out, status), A); }
  { auto c = chan; c[31] = -1; expect("chan = -1", call(depth, labels, B, S, NC, c.data(), dch.data(), NCH, ws, out, status), A); }
  { auto d = dch; d[1] = -2; expect("dch = -2", call(depth, labels, B, S, NC, chan.data(), d.data(), NCH, ws, out, status), A); }
  { auto d = dch; d[4] = 29; expect("dch = nch - 41", call(depth, labels, B, S, NC, chan.data(), d.data(), NCH, ws, out, status), A); }
  { auto d = dch; d[4] = 1 << 30; expect("dch = 2^30", call(depth, labels, B, S, NC, chan.data(), d.data(), NCH, ws, out, status), A); }
  { auto d = dch; d[5] = d[4]; expect("a depth channel owned twice", call(depth, labels, B, S, NC, chan.data(), d.data(), NCH, ws, out, status), A); }
  if (sln_observed_target_workspace_bytes(B, 6) != U || sln_observed_target_workspace_bytes(0, S) != U || sln_observed_target_workspace_bytes(B, S) <= 0) {
    std::printf("FAIL workspace bytes\n"); ++failures;
  }
}

// the frame sizes every face, compose and fuse call refuses: (B or R, Hs, Ws); 2 * 4096 * 2049 faces are 8192 more than 2^24
struct Frames { const char* what; int B, Hs, Ws; };
static const Frames BAD_FRAMES[] = {{"B = 0", 0, 3, 4}, {"B = -1", -1, 3, 4}, {"B = 65536", 65536, 3, 4}, {"Hs = 1", 2, 1, 4}, {"Ws = 1", 2, 3, 1},
                                    {"Hs = 0", 2, 0, 4}, {"Ws = -5", 2, 3, -5}, {"F > 2^24", 2, 4097, 2050}};

static void faces_checks() {
  const SlnReproject good = {depth, kk, pose, K, 2, 3, 4, 0, 512.0f, 0.1f, 0.05f, 0.0f};
  auto with = [&](auto&& change, float* fx = out) { SlnReproject d = good; change(d); return sln_reproject_faces(&d, fx, nullptr); };
  expect("faces: null descriptor", sln_reproject_faces(nullptr, out, nullptr), A);
  expect("faces: null faces_xyz", with([](SlnReproject&) {}, nullptr), A);
  expect("faces: null depth_src", with([](SlnReproject& d) { d.depth_src = nullptr; }), A);
  expect("faces: null k_src", with([](SlnReproject& d) { d.k_src = nullptr; }), A);
  expect("faces: null pose", with([](SlnReproject& d) { d.pose = nullptr; }), A);
  expect("faces: null K_tgt", with([](SlnReproject& d) { d.K_tgt = nullptr; }), A);
  for (const Frames& f : BAD_FRAMES) {
    std::printf("     faces, %s: ", f.what);
    expect("refused", with([&](SlnReproject& d) { d.B = f.B; d.Hs = f.Hs; d.Ws = f.Ws; }), A);
  }
  for (float v : {0.0f, -512.0f, NaN}) {
    std::printf("     faces, value %g: ", v);
    expect("orig_size", with([&](SlnReproject& d) { d.orig_size = v; }), A);
    expect("near", with([&](SlnReproject& d) { d.near = v; }), A);
    if (v != 0.0f) expect("gap", with([&](SlnReproject& d) { d.gap = v; }), A);
  }
  expect("faces: faces_xyz 4 bytes off", with([](SlnReproject&) {}, out + 1), A);
}

static void compose_checks() {
  auto call = [&](const int32_t* f, const float* w, const float* rd, const unsigned char* l, int B, int Hs, int Ws, int S, float* d,
                  unsigned char* lo, int64_t* h) { return sln_reproject_compose(f, w, rd, l, B, Hs, Ws, S, d, lo, h, nullptr); };
  expect("compose: null face_index", call(nullptr, wgt, depth, labels, 2, 3, 4, 8, out, lout, hits), A);
  expect("compose: null weight", call(fi, nullptr, depth, labels, 2, 3, 4, 8, out, lout, hits), A);
  expect("compose: null raster_depth", call(fi, wgt, nullptr, labels, 2, 3, 4, 8, out, lout, hits), A);
  expect("compose: null labels_src", call(fi, wgt, depth, nullptr, 2, 3, 4, 8, out, lout, hits), A);
  expect("compose: null depth_out", call(fi, wgt, depth, labels, 2, 3, 4, 8, nullptr, lout, hits), A);
  expect("compose: null labels_out", call(fi, wgt, depth, labels, 2, 3, 4, 8, out, nullptr, hits), A);
  expect("compose: null hits", call(fi, wgt, depth, labels, 2, 3, 4, 8, out, lout, nullptr), A);
  for (const Frames& f : BAD_FRAMES) {
    std::printf("     compose, %s: ", f.what);
    expect("refused", call(fi, wgt, depth, labels, f.B, f.Hs, f.Ws, 8, out, lout, hits), A);
  }
  for (int S : {0, -8, 4097}) {
    std::printf("     compose, S = %d: ", S);
    expect("refused", call(fi, wgt, depth, labels, 2, 3, 4, S, out, lout, hits), A);
  }
  expect("compose: hits 4 bytes off", call(fi, wgt, depth, labels, 2, 3, 4, 8, out, lout, off(hits, 4)), A);
}

static void fuse_checks() {
  struct Args {
    const int32_t* f = fi; const float* w = wgt; const float* rd = depth; const unsigned char* l = labels;
    int R = 2, V = 3, Hs = 3, Ws = 4, S = 8; float gap = 0.05f;
    float* d = out; unsigned char* lo = lout; unsigned char* so = u8a; unsigned char* co = u8b; unsigned char* ao = u8c;
    int64_t* h = hits; int64_t* wn = wins;
  };
  auto with = [&](auto&& change) {
    Args a; change(a);
    return sln_reproject_fuse(a.f, a.w, a.rd, a.l, a.R, a.V, a.Hs, a.Ws, a.S, a.gap, a.d, a.lo, a.so, a.co, a.ao, a.h, a.wn, nullptr);
  };
  expect("fuse: null face_index", with([](Args& a) { a.f = nullptr; }), A);
  expect("fuse: null weight", with([](Args& a) { a.w = nullptr; }), A);
  expect("fuse: null raster_depth", with([](Args& a) { a.rd = nullptr; }), A);
  expect("fuse: null labels_src", with([](Args& a) { a.l = nullptr; }), A);
  expect("fuse: null depth_out", with([](Args& a) { a.d = nullptr; }), A);
  expect("fuse: null labels_out", with([](Args& a) { a.lo = nullptr; }), A);
  expect("fuse: null hits", with([](Args& a) { a.h = nullptr; }), A);
  for (const Frames& f : BAD_FRAMES) {
    std::printf("     fuse, R as %s: ", f.what);
    expect("refused", with([&](Args& a) { a.R = f.B; a.V = 1; a.Hs = f.Hs; a.Ws = f.Ws; }), A);
  }
  expect("fuse: V = 0", with([](Args& a) { a.V = 0; }), A);
  expect("fuse: V = -3", with([](Args& a) { a.V = -3; }), A);
  expect("fuse: V = 256", with([](Args& a) { a.V = 256; }), A);
  expect("fuse: R = -2, V = -3", with([](Args& a) { a.R = -2; a.V = -3; }), A);
  expect("fuse: R * V = 258 * 255 = 65790", with([](Args& a) { a.R = 258; a.V = 255; }), A);
  expect("fuse: R * V = 2^31 - 1 frames times 255", with([](Args& a) { a.R = 0x7fffffff; a.V = 255; }), A);
  for (int S : {0, -8, 4097}) {
    std::printf("     fuse, S = %d: ", S);
    expect("refused", with([&](Args& a) { a.S = S; }), A);
  }
  expect("fuse: gap < 0", with([](Args& a) { a.gap = -0.01f; }), A);
  expect("fuse: gap NaN", with([](Args& a) { a.gap = NaN; }), A);
  expect("fuse: hits 4 bytes off", with([](Args& a) { a.h = off(hits, 4); }), A);
  expect("fuse: wins 4 bytes off", with([](Args& a) { a.wn = off(wins, 4); }), A);
  expect("fuse: depth_out 2 bytes off", with([](Args& a) { a.d = off(out, 2); }), A);
}

static void prefilter_checks() {
  struct Args {
    const float* d = depth; const unsigned char* l = labels; const float* k = kk;
    int B = 2, Hs = 5, Ws = 6, f = 2; float gap = 0.05f;
    float* dd = out; unsigned char* lo = lout; float* ko = K; int64_t* c = counts;
  };
  auto with = [&](auto&& change) {
    Args a; change(a);
    return sln_observed_prefilter(a.d, a.l, a.k, a.B, a.Hs, a.Ws, a.f, a.gap, a.dd, a.lo, a.ko, a.c, nullptr);
  };
  expect("prefilter: null depth_src", with([](Args& a) { a.d = nullptr; }), A);
  expect("prefilter: null labels_src", with([](Args& a) { a.l = nullptr; }), A);
  expect("prefilter: null k_src", with([](Args& a) { a.k = nullptr; }), A);
  expect("prefilter: null depth_out", with([](Args& a) { a.dd = nullptr; }), A);
  expect("prefilter: null labels_out", with([](Args& a) { a.lo = nullptr; }), A);
  expect("prefilter: null k_out", with([](Args& a) { a.ko = nullptr; }), A);
  expect("prefilter: B = 0", with([](Args& a) { a.B = 0; }), A);
  expect("prefilter: B = -1", with([](Args& a) { a.B = -1; }), A);
  expect("prefilter: B = 65536", with([](Args& a) { a.B = 65536; }), A);
  expect("prefilter: f = 0", with([](Args& a) { a.f = 0; }), A);
  expect("prefilter: f = -2", with([](Args& a) { a.f = -2; }), A);
  expect("prefilter: f = 9", with([](Args& a) { a.f = 9; a.Hs = a.Ws = 64; }), A);
  expect("prefilter: Hs < f", with([](Args& a) { a.Hs = 1; }), A);
  expect("prefilter: Ws < f", with([](Args& a) { a.Ws = 1; }), A);
  expect("prefilter: Hs = 0 at f = 1", with([](Args& a) { a.f = 1; a.Hs = 0; }), A);
  expect("prefilter: 2^19 x 2^13 = 2^32 tiles", with([](Args& a) { a.f = 1; a.Hs = 1 << 20; a.Ws = 1 << 18; }), A);
  expect("prefilter: gap < 0", with([](Args& a) { a.gap = -0.01f; }), A);
  expect("prefilter: gap NaN", with([](Args& a) { a.gap = NaN; }), A);
  expect("prefilter: counts 4 bytes off", with([](Args& a) { a.c = off(counts, 4); }), A);
  expect("prefilter: depth_src 2 bytes off", with([](Args& a) { a.d = off(depth, 2); }), A);
  expect("prefilter: depth_out 2 bytes off", with([](Args& a) { a.dd = off(out, 2); }), A);
  expect("prefilter: k_src 2 bytes off", with([](Args& a) { a.k = off(kk, 2); }), A);
  expect("prefilter: k_out 2 bytes off", with([](Args& a) { a.ko = off(K, 2); }), A);
}

int main() {
  target_checks();
  prefilter_checks();
  faces_checks();
  compose_checks();
  fuse_checks();
  std::printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}
