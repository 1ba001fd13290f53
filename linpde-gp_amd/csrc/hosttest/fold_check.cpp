// Stand-alone host check of csrc/fold_table.h (tests/test_cv_host.py builds it with AddressSanitizer + UBSan and runs it): every
// entry of the fold table against its literal formula -- padded row = padded offset of the row's block + row within the block --
// from a brute-force walk over the fold map; ragged blocks, rows in no fold, folds on both sides of the 128-row threshold, the
// batches of the tile folds, and the refusals.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fold_table.h"

using lpgp::FoldTable;

static int failures = 0;

static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  if (ok) return;
  ++failures;
  std::printf("fold_check: %s (%lld, %lld)\n", what, a, b);
}

// blocks of the given sizes, each padded to the next multiple of 128, as lpgp_mat_add_block lays them out
static std::vector<lpgp_block> layout(const std::vector<int64_t>& sizes) {
  std::vector<lpgp_block> out;
  int64_t off = 0, poff = 0;
  for (int64_t n : sizes) {
    out.push_back(lpgp_block{n, off, poff, (n + 127) / 128 * 128});
    off += n;
    poff += (n + 127) / 128 * 128;
  }
  return out;
}

// the literal formula, by a search for the block of logical row i
static int64_t padded_row(const std::vector<lpgp_block>& blocks, int64_t i) {
  for (const lpgp_block& b : blocks)
    if (i >= b.off && i < b.off + b.n) return b.poff + (i - b.off);
  return -1;
}

static void check_table(const std::vector<int64_t>& sizes, const std::vector<int32_t>& fold_of, int32_t nfolds) {
  const std::vector<lpgp_block> blocks = layout(sizes);
  const int64_t n = (int64_t)fold_of.size();
  FoldTable t;
  std::string err;
  const int rc = lpgp::fold_table_build(blocks.data(), (int)blocks.size(), fold_of.data(), n, nfolds, &t, &err);
  expect(rc == 0, err.c_str(), rc);
  if (rc != 0) return;
  expect(t.nfolds == nfolds && (int64_t)t.start.size() == nfolds + 1 && t.start[0] == 0, "start", nfolds);
  expect(t.lrow.size() == t.prow.size() && t.members() == t.start.back(), "members", t.members());
  int64_t members = 0, cov = 0, tcov = 0;
  size_t nt = 0, nl = 0;
  for (int32_t f = 0; f < nfolds; ++f) {
    // brute force: the rows of fold f in increasing Gram order
    std::vector<int64_t> rows;
    for (int64_t i = 0; i < n; ++i)
      if (fold_of[(size_t)i] == f) rows.push_back(i);
    expect(t.size(f) == (int32_t)rows.size(), "fold size", f, t.size(f));
    if (t.size(f) != (int32_t)rows.size()) return;
    for (size_t k = 0; k < rows.size(); ++k) {
      const size_t at = (size_t)t.start[(size_t)f] + k;
      expect(t.lrow[at] == rows[k], "logical row", f, (long long)k);
      expect(t.prow[at] == padded_row(blocks, rows[k]), "padded row", f, (long long)k);
      if (k > 0) expect(t.prow[at] > t.prow[at - 1], "padded rows increase", f, (long long)k);
    }
    expect(t.cov_off[(size_t)f] == cov, "covariance offset", f, t.cov_off[(size_t)f]);
    const int64_t b = (int64_t)rows.size();
    cov += b * b;
    if (b <= 128) {
      expect(nt < t.tile.size() && t.tile[nt] == f, "tile fold list", f);
      expect(nt < t.tile_cov_off.size() && t.tile_cov_off[nt] == tcov, "tile covariance offset", f);
      tcov += b * b;
      ++nt;
    } else {
      expect(nl < t.large.size() && t.large[nl] == f, "large fold list", f);
      ++nl;
    }
    members += b;
  }
  expect(nt == t.tile.size() && nl == t.large.size(), "fold lists", (long long)nt, (long long)nl);
  expect(t.cov_off.back() == cov && t.tile_cov_off.size() == nt + 1 && t.tile_cov_off.back() == tcov, "covariance totals", cov, tcov);
  int64_t unassigned = 0;
  for (int32_t f : fold_of) unassigned += f < 0;
  expect(members + unassigned == n && t.members() == members, "every row is in its fold or in none", members, unassigned);
}

static void check_batches(int64_t ntile, int64_t batch) {
  const int64_t nb = lpgp::fold_num_batches(ntile, batch);
  expect(nb == (ntile + batch - 1) / batch, "number of batches", ntile, batch);
  int64_t next = 0;
  for (int64_t k = 0; k < nb; ++k) {
    int64_t first, count;
    lpgp::fold_batch(ntile, batch, k, &first, &count);
    expect(first == next && count >= 1 && count <= batch, "batch", k, count);
    if (k + 1 < nb) expect(count == batch, "only the last batch is ragged", k, count);
    next = first + count;
  }
  expect(next == ntile, "the batches cover the tile folds", next, ntile);
  int64_t first, count;
  lpgp::fold_batch(ntile, batch, nb, &first, &count);
  expect(count == 0, "a batch past the end is empty", nb, count);
}

static void check_refusal(const std::vector<int64_t>& sizes, const std::vector<int32_t>& fold_of, int32_t nfolds, const char* needle) {
  std::vector<lpgp_block> blocks = layout(sizes);
  FoldTable t;
  t.nfolds = -7;                                 // must stay as it is
  std::string err;
  const int rc = lpgp::fold_table_build(blocks.data(), (int)blocks.size(), fold_of.data(), (int64_t)fold_of.size(), nfolds, &t, &err);
  expect(rc == -2, "a refusal returns -2", rc);
  expect(err.find(needle) != std::string::npos, needle);
  expect(t.nfolds == -7 && t.start.empty(), "a refused table is not written");
}

int main() {
  static_assert(FoldTable::TB == 128, "the tile edge");
  // 150 + 70 rows in 256 + 128 padded: the map has a gap at 150 .. 255
  {
    std::vector<int32_t> fo(220);
    for (int i = 0; i < 220; ++i) fo[(size_t)i] = i % 7 == 3 ? -1 : (i * 37 % 220) % 5;     // five folds across both blocks, some rows in none
    check_table({150, 70}, fo, 5);
    for (int i = 0; i < 220; ++i) fo[(size_t)i] = i;                                         // singletons
    check_table({150, 70}, fo, 220);
    for (int i = 0; i < 220; ++i) fo[(size_t)i] = 0;                                         // one fold of all rows: large
    check_table({150, 70}, fo, 1);
    for (int i = 0; i < 220; ++i) fo[(size_t)i] = i < 128 ? 1 : (i < 128 + 129 - 40 ? -1 : 0);
    check_table({150, 70}, fo, 2);
    for (int i = 0; i < 220; ++i) fo[(size_t)i] = i < 150 ? 0 : 1;                           // "blocks": 150 large, 70 tile
    check_table({150, 70}, fo, 2);
  }
  // exactly 128 and 129 rows, the rest in no fold; ragged blocks 1, 128, 129, 5 (tails of 127, 0, 127, 123 padded rows)
  {
    std::vector<int32_t> fo(263, -1);
    for (int i = 0; i < 128; ++i) fo[(size_t)(2 * i)] = 1;
    for (int i = 0; i < 129; ++i) fo[(size_t)(2 * i + 1)] = 0;
    check_table({1, 128, 129, 5}, fo, 2);
    check_table({263}, fo, 2);
  }
  check_batches(220, 3);                         // 74 batches, the last of one fold
  check_batches(220, 512);
  check_batches(512, 512);
  check_batches(513, 512);
  check_batches(1, 1);
  expect(lpgp::fold_num_batches(220, 3) == 74, "220 folds in batches of 3");
  // refusals
  {
    std::vector<int32_t> fo(220, 0);
    fo[17] = 2;
    check_refusal({150, 70}, fo, 2, "fold_of[17] = 2 is outside -1 .. 1");
    fo[17] = -2;
    check_refusal({150, 70}, fo, 2, "fold_of[17] = -2 is outside");
    fo[17] = 0;
    check_refusal({150, 70}, fo, 2, "fold 1 is empty");
    fo.assign(220, -1);
    check_refusal({150, 70}, fo, 1, "fold 0 is empty");
    fo.assign(219, 0);
    check_refusal({150, 70}, fo, 1, "the blocks hold 220 rows, not 219");
    fo.assign(220, 0);
    check_refusal({150, 70}, fo, 0, "bad argument");
  }
  if (failures) {
    std::printf("fold_check: %d checks failed\n", failures);
    return 1;
  }
  std::printf("fold_check: all checks passed\n");
  return 0;
}
