// The fold table of lpgp_mat_cv (evidence_cv.hip): which rows of the padded matrix make up each cross-validation fold.  Plain
// C++17, no HIP: csrc/hosttest/fold_check.cpp holds every entry to its literal formula on the host -- padded row = padded offset
// of the row's block + row within the block.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "mat_state.h"

namespace lpgp {

// The members of fold f are entries [start[f], start[f + 1]) of lrow / prow, in increasing Gram order (so in increasing padded
// order too: the map logical -> padded row is monotone).  Folds of at most TB rows go through the tile kernels, many per launch;
// a larger one is handled on its own.
struct FoldTable {
  static constexpr int32_t TB = 128;             // == TILE (lpgp_desc.h)
  int32_t nfolds = 0;
  std::vector<int32_t> start;                    // nfolds + 1
  std::vector<int32_t> lrow;                     // logical (Gram) row of every member
  std::vector<int32_t> prow;                     // its row in the padded layout
  std::vector<int32_t> tile;                     // the folds of at most TB rows, in fold order
  std::vector<int32_t> large;                    // the others, in fold order
  std::vector<int64_t> cov_off;                  // nfolds + 1: where fold f's b_f x b_f covariance starts among all of them (doubles)
  std::vector<int64_t> tile_cov_off;             // tile.size() + 1: the same among the covariances of the tile folds alone
  int32_t size(int32_t f) const { return start[(size_t)f + 1] - start[(size_t)f]; }
  int64_t members() const { return (int64_t)prow.size(); }
};

// 0, or -2 with *err set: a block list that is not a partition of [0, n) into padded slots, an entry of fold_of outside
// -1 .. nfolds - 1, an empty fold.  *out is written only on success.
inline int fold_table_build(const lpgp_block* blocks, int nblocks, const int32_t* fold_of, int64_t n, int32_t nfolds, FoldTable* out, std::string* err) {
  auto fail = [&](const std::string& msg) {
    if (err) *err = msg;
    return -2;
  };
  if (!blocks || nblocks < 1 || !fold_of || !out || n < 1 || nfolds < 1) return fail("fold table: bad argument");
  int64_t off = 0, poff = 0;
  for (int b = 0; b < nblocks; ++b) {
    const lpgp_block& B = blocks[b];
    if (B.n < 1 || B.off != off || B.poff < poff || B.poff % FoldTable::TB != 0)
      return fail("fold table: block " + std::to_string(b) + " does not continue the layout");
    off += B.n;
    poff = B.poff + (B.n + FoldTable::TB - 1) / FoldTable::TB * FoldTable::TB;
  }
  if (off != n || poff > (int64_t)INT32_MAX) return fail("fold table: the blocks hold " + std::to_string(off) + " rows, not " + std::to_string(n));
  FoldTable t;
  t.nfolds = nfolds;
  t.start.assign((size_t)nfolds + 1, 0);
  int64_t members = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int32_t f = fold_of[i];
    if (f < -1 || f >= nfolds)
      return fail("fold_of[" + std::to_string(i) + "] = " + std::to_string(f) + " is outside -1 .. " + std::to_string(nfolds - 1));
    if (f >= 0) {
      ++t.start[(size_t)f + 1];
      ++members;
    }
  }
  for (int32_t f = 0; f < nfolds; ++f) {
    if (t.start[(size_t)f + 1] == 0) return fail("fold " + std::to_string(f) + " is empty");
    t.start[(size_t)f + 1] += t.start[(size_t)f];
  }
  t.lrow.assign((size_t)members, 0);
  t.prow.assign((size_t)members, 0);
  std::vector<int32_t> next(t.start.begin(), t.start.end() - 1);
  for (int b = 0; b < nblocks; ++b)
    for (int64_t i = 0; i < blocks[b].n; ++i) {
      const int32_t f = fold_of[blocks[b].off + i];
      if (f < 0) continue;
      const size_t at = (size_t)next[(size_t)f]++;
      t.lrow[at] = (int32_t)(blocks[b].off + i);
      t.prow[at] = (int32_t)(blocks[b].poff + i);
    }
  t.cov_off.assign((size_t)nfolds + 1, 0);
  t.tile_cov_off.assign(1, 0);
  for (int32_t f = 0; f < nfolds; ++f) {
    const int64_t b = t.size(f);
    t.cov_off[(size_t)f + 1] = t.cov_off[(size_t)f] + b * b;
    if (b <= FoldTable::TB) {
      t.tile.push_back(f);
      t.tile_cov_off.push_back(t.tile_cov_off.back() + b * b);
    } else {
      t.large.push_back(f);
    }
  }
  *out = std::move(t);
  return 0;
}

// the tile folds run in batches of `batch`: batch k covers entries [first, first + count) of FoldTable::tile; the last may be ragged
inline int64_t fold_num_batches(int64_t ntile, int64_t batch) { return batch < 1 ? 0 : (ntile + batch - 1) / batch; }
inline void fold_batch(int64_t ntile, int64_t batch, int64_t k, int64_t* first, int64_t* count) {
  *first = k * batch;
  *count = *first >= ntile ? 0 : (ntile - *first < batch ? ntile - *first : batch);
}

}  // namespace lpgp
