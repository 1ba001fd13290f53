// The two operands of the single-GPU factorisation and substitution drivers (potrf.hip, chain.hip, trsv.hip) by 128-tiles: every
// tile address of those drivers is formed here, in int64.  Plain C++17, no HIP: csrc/hosttest/view_check.cpp holds the offsets
// to their literal formulae on the host.  Trivially copyable, passed by value.
#pragma once

#include <cstdint>

namespace lpgp {

// the lower factor (or the matrix being factored) of a single-GPU matrix: column-major, leading dimension ld
struct FactorView {
  static constexpr int64_t TB = 128;             // == TILE (lpgp_desc.h)
  double* a;                                     // tile (0, 0)
  double* linv;                                  // inverse of diagonal tile 0; the others follow, 128 x 128 each
  int64_t ld;
  static int64_t off(int64_t ld, int i, int j) { return (int64_t)i * TB + (int64_t)j * TB * ld; }     // element offset of tile (i, j)
  double* tile(int i, int j) const { return a + off(ld, i, j); }
  double* diag(int k) const { return a + off(ld, k, k); }
  double* inv(int k) const { return linv + (int64_t)k * TB * TB; }
  FactorView trailing(int t0) const { return {diag(t0), inv(t0), ld}; }      // L[t0:, t0:]
};

// a right-hand side V: padded rows x (mtl * 128) columns, column-major
struct RhsView {
  double* v;
  int64_t ld;
  int mtl;                                       // tile columns
  double* rows(int t) const { return v + (int64_t)t * FactorView::TB; }      // tile row t, first column
  RhsView cols(int c0, int c1) const { return {v + (int64_t)c0 * FactorView::TB * ld, ld, c1 - c0}; }    // tile columns [c0, c1)
};

}  // namespace lpgp
