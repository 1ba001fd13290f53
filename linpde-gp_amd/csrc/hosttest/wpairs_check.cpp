// Stand-alone check of the pair-list validation of the variable-coefficient assembly (lower.cpp: check_wpairs), meant to
// be built with the host compiler and -fsanitize=address,undefined and run directly:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I../../include -I.. wpairs_check.cpp ../lower.cpp
// Every list lives on the heap at its exact size, so a read past its end is caught.  Exit status 0: every case behaved.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../lpgp_desc.h"

using namespace lpgp;

static int g_fail = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s (last error: %s)\n", what, last_error());
    ++g_fail;
  }
}

static std::vector<lpgp_wpair> grid(const lpgp_kdesc* kd, int A0, int A1) {
  std::vector<lpgp_wpair> v;
  for (int a = 0; a < A0; ++a)
    for (int b = 0; b < A1; ++b) v.push_back(lpgp_wpair{kd, 1, a, b});
  v.shrink_to_fit();
  return v;
}

int main() {
  std::unique_ptr<lpgp_kdesc> kd2(new lpgp_kdesc()), kd3(new lpgp_kdesc());
  kd2->d = 2;
  kd3->d = 3;
  const char* fn = "wpairs_check";
  {
    auto v = grid(kd2.get(), 3, 2);
    expect(check_wpairs(v.data(), (int)v.size(), 3, 2, WP_RECT, fn) == 0, "3 x 2 rectangular list");
    expect(check_wpairs(v.data(), (int)v.size(), 2, 2, WP_RECT, fn) != 0 && std::strstr(last_error(), "row weight index"), "row index out of range");
    expect(check_wpairs(v.data(), (int)v.size(), 3, 1, WP_RECT, fn) != 0 && std::strstr(last_error(), "column weight index"), "column index out of range");
    expect(check_wpairs(v.data(), (int)v.size(), 5, 2, WP_RECT, fn) != 0, "A0 above the cap");
    expect(check_wpairs(v.data(), (int)v.size(), 3, 5, WP_RECT, fn) != 0, "A1 above the cap");
    expect(check_wpairs(v.data(), 0, 3, 2, WP_RECT, fn) != 0 && check_wpairs(v.data(), 17, 3, 2, WP_RECT, fn) != 0, "npairs outside 1 .. 16");
    expect(check_wpairs(nullptr, 1, 1, 1, WP_RECT, fn) != 0, "null list");
    expect(check_wpairs(v.data(), (int)v.size(), 3, 0, WP_RECT, fn) != 0 && std::strstr(last_error(), "column weight functions"), "A1 = 0 off the diagonal");
  }
  {
    auto v = grid(kd2.get(), 4, 4);                                     // the largest list: 16 pairs
    expect(check_wpairs(v.data(), 16, 4, 0, WP_SYM, fn) == 0, "4 x 4 symmetric list");
    v.pop_back();                                                       // (3, 3) gone: still symmetric
    v.shrink_to_fit();
    expect(check_wpairs(v.data(), 15, 4, 0, WP_SYM, fn) == 0, "symmetric list without one diagonal pair");
    v.erase(v.begin() + 1);                                             // (0, 1) gone, (1, 0) still there
    v.shrink_to_fit();
    expect(check_wpairs(v.data(), 14, 4, 0, WP_SYM, fn) != 0 && std::strstr(last_error(), "symmetric"), "asymmetric diagonal list");
  }
  {
    auto v = grid(kd2.get(), 2, 1);
    expect(check_wpairs(v.data(), 2, 2, 1, WP_CROSS, fn) == 0, "cross list");
    v[1].b = 1;
    expect(check_wpairs(v.data(), 2, 2, 1, WP_CROSS, fn) != 0, "cross list with b != 0");
    v[1].b = 0;
    v[1].kd = kd3.get();
    expect(check_wpairs(v.data(), 2, 2, 1, WP_CROSS, fn) != 0 && std::strstr(last_error(), "input dimension"), "mixed input dimensions");
    v[1].kd = nullptr;
    expect(check_wpairs(v.data(), 2, 2, 1, WP_CROSS, fn) != 0, "null descriptor");
    v[1].kd = kd2.get();
    v[1].ngroups = 0;
    expect(check_wpairs(v.data(), 2, 2, 1, WP_CROSS, fn) != 0, "ngroups = 0");
  }
  std::printf(g_fail ? "%d case(s) failed\n" : "wpairs_check: all cases passed\n", g_fail);
  return g_fail ? 1 : 0;
}
