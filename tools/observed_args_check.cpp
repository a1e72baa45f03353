// The argument checks of sln_observed_target, run from a program of their own so that the host code can be built with a sanitizer
// (never load a sanitized library into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude -I3d_sln_amd/csrc \
//         tools/observed_args_check.cpp 3d_sln_amd/csrc/observed_target.hip -o observed_args_check && ./observed_args_check
//
// Every call below must be refused before anything is launched: the "device" pointers are small host arrays that a correct check never
// dereferences, the host tables are sized exactly NC entries, so a read past a table is the sanitizer's to report.  Needs no GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sln_hip.h"

static int failures = 0;

static void expect(const char* what, int rc, int want) {
  if (rc != want) { std::printf("FAIL %s: returned %d, expected %d\n", what, rc, want); ++failures; }
  else std::printf("ok   %s\n", what);
}

int main() {
  const int NC = 32, NCH = 70, B = 2, S = 8;
  std::vector<int32_t> chan(NC), dch(NC);
  for (int c = 0; c < NC; ++c) { chan[c] = c; dch[c] = c < 3 ? -1 : c - 3; }
  alignas(16) static float depth[64], out[64];
  alignas(16) static unsigned char labels[64];
  alignas(16) static int32_t ws[64], status[4];
  auto call = [&](const float* d, const unsigned char* l, int b, int s, int nc, const int32_t* ch, const int32_t* dc, int nch, void* w, float* o,
                  int32_t* st) { return sln_observed_target(d, l, b, s, nc, ch, dc, nch, w, o, st, nullptr); };
  const int U = SLN_E_UNSUPPORTED, A = SLN_E_BADARG;

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
  std::printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}
