// The argument checks of sln_view_place_project / sln_view_compose, run from a program of their own so that the host code can be built
// with a sanitizer (never load a sanitized library into python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude -I3d_sln_amd/csrc \
//         tools/view_args_check.cpp 3d_sln_amd/csrc/shade_view.hip -o view_args_check && ./view_args_check
//
// Every call below must be refused with SLN_E_BADARG before anything is launched: the "device" pointers are small host arrays that a
// correct check never dereferences, the host tables are sized exactly, so a read past a table is the sanitizer's to report.  Needs no GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sln_hip.h"

static int failures = 0;

static void expect_badarg(const char* what, int rc) {
  if (rc != -1) { std::printf("FAIL %s: returned %d, expected SLN_E_BADARG (-1)\n", what, rc); ++failures; }
  else std::printf("ok   %s\n", what);
}

int main() {
  const int M = 3, Fm = 12, Vs = 8, Fs = 4;
  std::vector<int32_t> voff = {0, 8, 16, 24}, foff = {0, 12, 24, 30}, shell_f(3 * Fs, 0);
  for (int i = 0; i < 3 * Fs; ++i) shell_f[i] = i % Vs;
  std::vector<float> dummy(64, 0.f);
  std::vector<int32_t> idummy(64, 0);
  std::vector<unsigned char> bdummy(64, 0);
  SlnViewPlace d{};
  d.bank_v = dummy.data(); d.bank_f = idummy.data(); d.voff = idummy.data(); d.foff = idummy.data();
  d.voff_host = voff.data(); d.foff_host = foff.data();
  d.A = dummy.data(); d.tr = dummy.data(); d.row_model = idummy.data(); d.row_label = bdummy.data();
  d.shell_v = dummy.data(); d.shell_f = idummy.data(); d.shell_f_host = shell_f.data(); d.shell_label = bdummy.data();
  d.K = dummy.data(); d.Rm = dummy.data(); d.t = dummy.data();
  d.M = M; d.Vtot = 24; d.Ftot = 30; d.Fm = Fm; d.Vs = Vs; d.Fs = Fs; d.R = 1; d.V = 1; d.N = 2;
  d.orig_size = 64.f; d.near = 0.1f;
  float* out = dummy.data();
  unsigned char* lab = bdummy.data();

  { SlnViewPlace e = d; e.Vtot = 23; expect_badarg("vertex table ends past the bank", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.Ftot = 29; expect_badarg("face table ends past the bank", sln_view_place_project(&e, out, lab, nullptr)); }
  { auto v = voff; v[2] = 7; SlnViewPlace e = d; e.voff_host = v.data(); expect_badarg("decreasing vertex table", sln_view_place_project(&e, out, lab, nullptr)); }
  { auto f = foff; f[0] = 1; SlnViewPlace e = d; e.foff_host = f.data(); expect_badarg("face table not from 0", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.Fm = 11; expect_badarg("a model with more faces than slots", sln_view_place_project(&e, out, lab, nullptr)); }
  { auto s = shell_f; s[3 * Fs - 1] = Vs; SlnViewPlace e = d; e.shell_f_host = s.data(); expect_badarg("shell corner past its vertices", sln_view_place_project(&e, out, lab, nullptr)); }
  { auto s = shell_f; s[0] = -1; SlnViewPlace e = d; e.shell_f_host = s.data(); expect_badarg("negative shell corner", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.R = 300; e.V = 300; expect_badarg("more views than a launch takes", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.N = 0; expect_badarg("no rows", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.orig_size = 0.f; expect_badarg("orig_size 0", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.voff_host = nullptr; expect_badarg("no host table", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.row_model = nullptr; expect_badarg("no row table", sln_view_place_project(&e, out, lab, nullptr)); }
  { SlnViewPlace e = d; e.N = 1 << 22; expect_badarg("more face slots than 2^24", sln_view_place_project(&e, out, lab, nullptr)); }
  expect_badarg("null descriptor", sln_view_place_project(nullptr, out, lab, nullptr));
  expect_badarg("null output", sln_view_place_project(&d, nullptr, lab, nullptr));

  std::vector<double> ws(16);
  double sum[4]; int64_t count[4];
  expect_badarg("compose: views do not divide the batch", sln_view_compose(idummy.data(), dummy.data(), lab, 3, 2, 4, 4, ws.data(), lab, out, sum, count, nullptr));
  expect_badarg("compose: no faces", sln_view_compose(idummy.data(), dummy.data(), lab, 2, 2, 0, 4, ws.data(), lab, out, sum, count, nullptr));
  expect_badarg("compose: unaligned workspace", sln_view_compose(idummy.data(), dummy.data(), lab, 2, 2, 4, 4, reinterpret_cast<char*>(ws.data()) + 4, lab, out, sum, count, nullptr));
  expect_badarg("compose: null map", sln_view_compose(nullptr, dummy.data(), lab, 2, 2, 4, 4, ws.data(), lab, out, sum, count, nullptr));
  if (sln_view_compose_workspace_bytes(0) >= 0 || sln_view_compose_workspace_bytes(2) != 2 * 128 * 16) { std::printf("FAIL workspace bytes\n"); ++failures; }
  std::printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}
