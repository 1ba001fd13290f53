// Stand-alone host check of csrc/factor_view.h (tests/test_view_host.py builds it with AddressSanitizer + UBSan and runs it):
// every address the views form, as an element offset from the view's base, against its literal formula in __int128.  Offsets
// only: nothing is dereferenced, and the base is a real object, so no pointer is formed from null.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "factor_view.h"

using lpgp::FactorView;
using lpgp::RhsView;
typedef __int128 wide;

static int failures = 0;
static double base_a[1], base_linv[1], base_v[1];

static wide elems(const double* p, const double* base) { return ((wide)(intptr_t)p - (wide)(intptr_t)base) / (wide)sizeof(double); }

static void expect(bool ok, const char* what, int64_t ld, int i, int j) {
  if (ok) return;
  ++failures;
  std::printf("view_check: %s wrong at ld = %lld, i = %d, j = %d\n", what, (long long)ld, i, j);
}

static wide off_ref(int64_t ld, int i, int j) { return (wide)i * 128 + (wide)j * 128 * (wide)ld; }

// tile rows / columns 0 .. T-1 of a factor with leading dimension ld: the listed tile indices, every pair of them with i >= j
static void check_factor(int64_t ld, std::initializer_list<int> idx) {
  const FactorView F{base_a, base_linv, ld};
  for (int i : idx)
    for (int j : idx) {
      if (i < j) continue;
      expect((wide)FactorView::off(ld, i, j) == off_ref(ld, i, j), "off", ld, i, j);
      expect(elems(F.tile(i, j), base_a) == off_ref(ld, i, j), "tile", ld, i, j);
      // the trailing sub-factor from t on, t every listed index up to j
      for (int t : idx) {
        if (t > j) continue;
        const FactorView S = F.trailing(t);
        expect(S.ld == ld, "trailing ld", ld, t, t);
        expect(elems(S.tile(i - t, j - t), S.a) == off_ref(ld, i, j) - off_ref(ld, t, t), "trailing tile", ld, i, j);
        expect(elems(S.tile(i - t, j - t), base_a) == off_ref(ld, i, j), "trailing tile (absolute)", ld, i, j);
        expect(elems(S.inv(i - t), S.linv) == ((wide)i - t) * 128 * 128, "trailing inv", ld, i, t);
        expect(elems(S.inv(i - t), base_linv) == (wide)i * 128 * 128, "trailing inv (absolute)", ld, i, t);
        expect(S.diag(j - t) == F.diag(j), "trailing diag", ld, j, t);
      }
    }
  for (int k : idx) {
    expect(elems(F.diag(k), base_a) == (wide)k * 128 * ((wide)ld + 1), "diag", ld, k, k);
    expect(elems(F.inv(k), base_linv) == (wide)k * 128 * 128, "inv", ld, k, k);
  }
}

static void check_rhs(int64_t ld, int mtl, std::initializer_list<int> rows, std::initializer_list<int> cols) {
  const RhsView V{base_v, ld, mtl};
  for (int t : rows) expect(elems(V.rows(t), base_v) == (wide)t * 128, "rows", ld, t, 0);
  for (int c0 : cols)
    for (int c1 : cols) {
      if (c1 < c0 || c1 > mtl) continue;
      const RhsView H = V.cols(c0, c1);
      expect(elems(H.v, base_v) == (wide)c0 * 128 * (wide)ld, "cols base", ld, c0, c1);
      expect(H.ld == ld && H.mtl == c1 - c0, "cols ld / mtl", ld, c0, c1);
      for (int t : rows) expect(elems(H.rows(t), base_v) == (wide)t * 128 + (wide)c0 * 128 * (wide)ld, "cols rows", ld, t, c0);
    }
}

int main() {
  static_assert(FactorView::TB == 128, "the tile edge");
  check_factor(128, {0});                                    // one tile
  check_factor(1536, {0, 1, 2, 3, 4, 7, 11});                // capacity == size: 12 tile rows
  check_factor(2688, {0, 1, 3, 4, 5, 11, 19});               // capacity (21 tile rows) larger than the matrix (20)
  check_factor(196608, {0, 1, 4, 511, 1024, 1534, 1535});    // element offset of tile (1535, 1535) > 2^35: an int intermediate shows
  expect(off_ref(196608, 1535, 1535) > ((wide)1 << 35), "the large case is not large", 196608, 1535, 1535);
  check_rhs(128, 1, {0}, {0, 1});
  check_rhs(2560, 9, {0, 1, 4, 19}, {0, 1, 4, 8, 9});
  check_rhs(196608, 1536, {0, 1, 1535}, {0, 1, 768, 1535, 1536});
  if (failures) {
    std::printf("view_check: %d checks failed\n", failures);
    return 1;
  }
  std::printf("view_check: all checks passed\n");
  return 0;
}
