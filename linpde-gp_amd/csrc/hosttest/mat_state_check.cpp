// Stand-alone host check of csrc/mat_state.h (tests/test_mat_state_host.py builds it with AddressSanitizer + UBSan and runs it): the
// block table and the factor state of a matrix handle walked through the life cycle the entry points of api.hip drive -- layout,
// enqueue and predict, check, views, rollback.  Every expected value is a literal, written down from what those entry points set
// by hand before the header existed; none is computed by the header.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mat_state.h"

using lpgp::MatState;

static int failures = 0;

#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      ++failures;                                                         \
      std::printf("mat_state_check: line %d: %s\n", __LINE__, #cond);     \
    }                                                                     \
  } while (0)

static bool block_is(const lpgp_block& b, int64_t n, int64_t off, int64_t poff, int64_t pn) {
  return b.n == n && b.off == off && b.poff == poff && b.pn == pn;
}
static bool sizes_are(const MatState& m, size_t view, size_t hidden, int64_t n, int64_t pn, int64_t pn_fact) {
  return m.blocks.size() == view && m.hidden.size() == hidden && m.n == n && m.pn == pn && m.pn_fact == pn_fact;
}
// has_w, has_r, unchecked, status_known
static bool flags_are(const MatState& m, int w, int r, int u, int k) { return m.has_w == w && m.has_r == r && m.unchecked == u && m.status_known == k; }

static MatState with_blocks(const std::vector<int64_t>& sizes) {
  MatState m;
  for (int64_t n : sizes) m.push_block(n);
  return m;
}

// lpgp_mat_check as api.hip drives the state: 0 with *info / *block, or -2 for a negative status (a timed-out hand-over)
static int check(MatState& m, int device_word, int* info, int* block) {
  *info = 0;
  *block = -1;
  if (!m.unchecked) return 0;
  const int h = m.status_known ? m.status_value : device_word;
  m.take_status(h);
  if (h < 0) return -2;
  *info = h;
  if (h > 0) *block = m.block_of_pivot(h);
  return 0;
}

static void check_layout() {
  MatState m;
  EXPECT(sizes_are(m, 0, 0, 0, 0, 0) && flags_are(m, 0, 0, 0, 0) && m.pn_fact_all == 0 && m.status_value == 0 && m.poisoned == 0);
  EXPECT(m.fully_factored() && m.total_blocks() == 0 && m.padded_end(0) == 0 && m.fact_all() == 0);
  EXPECT(block_is(m.next_block(1), 1, 0, 0, 128) && sizes_are(m, 0, 0, 0, 0, 0));        // a query: nothing pushed
  EXPECT(m.push_block(1) == 0);
  m.weights_resident();
  m.residual_resident();
  EXPECT(flags_are(m, 1, 1, 0, 0));
  EXPECT(m.push_block(128) == 1);
  EXPECT(flags_are(m, 0, 0, 0, 0));              // weights and residual were those of the smaller matrix
  EXPECT(block_is(m.next_block(129), 129, 129, 256, 256));
  EXPECT(m.push_block(129) == 2);
  EXPECT(m.push_block(300) == 3);
  EXPECT(block_is(m.blocks[0], 1, 0, 0, 128));
  EXPECT(block_is(m.blocks[1], 128, 1, 128, 128));
  EXPECT(block_is(m.blocks[2], 129, 129, 256, 256));
  EXPECT(block_is(m.blocks[3], 300, 258, 512, 384));
  EXPECT(sizes_are(m, 4, 0, 558, 896, 0) && !m.fully_factored() && m.total_blocks() == 4);
  EXPECT(m.padded_end(1) == 128 && m.padded_end(2) == 256 && m.padded_end(3) == 512 && m.padded_end(4) == 896);
  // logical <-> padded: the literal block table above, searched row by row
  static const int64_t N[4] = {1, 128, 129, 300}, OFF[4] = {0, 1, 129, 258}, POFF[4] = {0, 128, 256, 512};
  auto logical_row = [&](int64_t p) -> int64_t {
    for (int b = 0; b < 4; ++b)
      if (p >= POFF[b] && p < POFF[b] + N[b]) return OFF[b] + (p - POFF[b]);
    return -1;
  };
  std::vector<double> x(558), padded(896, -7.0), back(558, -3.0);
  for (size_t i = 0; i < x.size(); ++i) x[i] = (double)(i + 1);
  m.scatter_padded(x.data(), padded.data());
  int64_t logical_rows = 0;
  for (int64_t p = 0; p < 896; ++p) {
    const int64_t l = logical_row(p);
    EXPECT(padded[(size_t)p] == (l < 0 ? 0.0 : (double)(l + 1)));
    logical_rows += l >= 0;
  }
  EXPECT(logical_rows == 558);
  m.gather_padded(padded.data(), back.data());
  EXPECT(back == x);
  for (int32_t sentinel : {-1, -5}) {            // (both callers fill -1 today; the padding rows are theirs)
    std::vector<int32_t> tab(896, sentinel);
    m.logical_of_padded(tab.data());
    for (int64_t p = 0; p < 896; ++p) EXPECT(tab[(size_t)p] == (logical_row(p) < 0 ? sentinel : (int32_t)logical_row(p)));
  }
  // ... of the VIEW: two blocks in view scatter 256 padded rows and no more
  m.factor_enqueued(false);
  std::string err;
  EXPECT(m.set_view(2, &err) == 0 && sizes_are(m, 2, 2, 129, 256, 256));
  std::vector<double> small(256 + 1, -7.0);
  m.scatter_padded(x.data(), small.data());
  EXPECT(small[0] == 1.0 && small[1] == 0.0 && small[127] == 0.0 && small[128] == 2.0 && small[255] == 129.0 && small[256] == -7.0);
}

static void check_enqueue_and_predict() {
  // eager: lpgp_potrf with status 129, then with status 0
  MatState m = with_blocks({129});
  m.weights_resident();
  m.residual_resident();
  m.factored(129);
  EXPECT(sizes_are(m, 1, 0, 129, 256, 0) && flags_are(m, 0, 0, 0, 0) && m.poisoned == 0);
  m.weights_resident();
  m.residual_resident();
  m.factored(0);
  EXPECT(sizes_are(m, 1, 0, 129, 256, 256) && flags_are(m, 0, 0, 0, 0) && m.fully_factored());
  // lpgp_potrf_enqueue drops the residual
  m.push_block(5);
  m.weights_resident();
  m.residual_resident();
  m.factor_enqueued(false);
  EXPECT(sizes_are(m, 2, 0, 134, 384, 384) && flags_are(m, 0, 0, 1, 0));
  // a prediction on that matrix (nothing fresh, a status owed): the status that comes back with the results is recorded
  m.residual_resident();
  m.status_stale();
  m.status_read_back(130);
  EXPECT(flags_are(m, 0, 1, 1, 1) && m.status_value == 130 && m.pn_fact == 384);
  // ... and lpgp_mat_check uses the recorded value, not the device word
  int info = -9, block = -9;
  EXPECT(check(m, 0, &info, &block) == 0 && info == 130 && block == 0);
  EXPECT(flags_are(m, 0, 1, 0, 0) && m.pn_fact == 384 && m.poisoned == 0);
  // a prediction on a checked matrix records nothing
  m.status_stale();
  m.status_read_back(7);
  EXPECT(flags_are(m, 0, 1, 0, 0) && m.status_value == 130);
  EXPECT(check(m, 7, &info, &block) == 0 && info == 0 && block == -1);
  // the fresh branch of lpgp_potrf_predict keeps the residual and drops the weights
  m.push_block(3);
  m.weights_resident();
  m.residual_resident();
  m.factor_enqueued(true);
  m.status_stale();
  m.status_read_back(0);
  EXPECT(sizes_are(m, 3, 0, 137, 512, 512) && flags_are(m, 0, 1, 1, 1) && m.status_value == 0);
  // status 0 clears the flags
  EXPECT(check(m, 55, &info, &block) == 0 && info == 0 && block == -1 && flags_are(m, 0, 1, 0, 0) && m.pn_fact == 512);
  // a status recorded earlier is void once another read-back is on its way
  m.status_pending();
  m.status_read_back(4);
  m.status_stale();
  EXPECT(flags_are(m, 0, 1, 1, 0));
  EXPECT(check(m, 257, &info, &block) == 0 && info == 257 && block == 1);
  // the capacity changed: the residual is gone, the weights are not
  m.weights_resident();
  m.storage_moved();
  EXPECT(flags_are(m, 1, 0, 0, 0));
}

static void check_check() {
  int info = -9, block = -9;
  std::string err;
  // pivot 130 is padded row 129: block 1 of the layout 1, 128, 129, 300 (padded rows 128 .. 255)
  MatState m = with_blocks({1, 128, 129, 300});
  m.factor_enqueued(false);
  EXPECT(check(m, 130, &info, &block) == 0 && info == 130 && block == 1);
  EXPECT(sizes_are(m, 4, 0, 558, 896, 896) && flags_are(m, 0, 0, 0, 0) && m.poisoned == 0);     // pn_fact still provisional
  m.weights_resident();
  m.residual_resident();
  m.status_pending();
  m.truncate(1);
  EXPECT(sizes_are(m, 1, 0, 1, 128, 128) && flags_are(m, 0, 0, 0, 0) && block_is(m.blocks[0], 1, 0, 0, 128));
  // ... also through a view that hides the block
  m = with_blocks({1, 128, 129, 300});
  m.factor_enqueued(false);
  EXPECT(m.set_view(1, &err) == 0 && sizes_are(m, 1, 3, 1, 128, 128) && m.unchecked == 1);
  EXPECT(check(m, 130, &info, &block) == 0 && info == 130 && block == 1);
  EXPECT(m.block_of_pivot(128) == 0 && m.block_of_pivot(129) == 1 && m.block_of_pivot(256) == 1 && m.block_of_pivot(257) == 2 &&
         m.block_of_pivot(896) == 3 && m.block_of_pivot(897) == -1 && m.block_of_pivot(0) == -1);
  EXPECT(m.set_view(-1, &err) == 0 && sizes_are(m, 4, 0, 558, 896, 896));
  // truncate to nothing
  m.truncate(0);
  EXPECT(sizes_are(m, 0, 0, 0, 0, 0) && flags_are(m, 0, 0, 0, 0));
  // a negative status: the matrix is dead, the status reported once (the entry points refuse a poisoned matrix from then on)
  m = with_blocks({1, 128});
  m.factor_enqueued(false);
  EXPECT(check(m, INT_MIN, &info, &block) == -2 && m.poisoned == 1 && flags_are(m, 0, 0, 0, 0));
  EXPECT(check(m, INT_MIN, &info, &block) == 0 && info == 0 && block == -1 && m.unchecked == 0 && m.poisoned == 1);
  m.truncate(1);
  EXPECT(m.poisoned == 1 && sizes_are(m, 1, 0, 1, 128, 128));
  MatState p;
  p.poison();
  EXPECT(p.poisoned == 1 && flags_are(p, 0, 0, 0, 0));
}

static void check_views() {
  std::string err;
  // five blocks -- padded offsets 0, 128, 256, 512, 640; 896 padded rows, 607 logical -- of which three are factored
  MatState m = with_blocks({100, 128, 200});
  m.factored(0);
  m.push_block(50);
  m.push_block(129);
  EXPECT(sizes_are(m, 5, 0, 607, 896, 512) && m.fact_all() == 512 && !m.fully_factored());
  EXPECT(m.set_view(2, &err) == 0);
  EXPECT(sizes_are(m, 2, 3, 228, 256, 256) && m.pn_fact_all == 512 && m.fact_all() == 512 && m.fully_factored() && m.total_blocks() == 5);
  EXPECT(block_is(m.block_at(1), 128, 100, 128, 128) && block_is(m.block_at(2), 200, 228, 256, 256) && block_is(m.block_at(4), 129, 478, 640, 256));
  EXPECT(m.padded_end(2) == 256 && m.padded_end(3) == 512 && m.padded_end(5) == 896);
  EXPECT(m.set_view(-1, &err) == 0);
  EXPECT(sizes_are(m, 5, 0, 607, 896, 512) && m.fact_all() == 512);
  EXPECT(block_is(m.blocks[2], 200, 228, 256, 256) && block_is(m.blocks[4], 129, 478, 640, 256));
  // refusals leave everything as it is
  m.weights_resident();
  m.residual_resident();
  EXPECT(m.set_view(4, &err) == -2 && err == "lpgp_mat_set_view: block 3 is not factored yet");
  EXPECT(m.set_view(0, &err) == -2 && err == "lpgp_mat_set_view: 0 of 5 blocks");
  EXPECT(m.set_view(6, &err) == -2 && err == "lpgp_mat_set_view: 6 of 5 blocks");
  EXPECT(sizes_are(m, 5, 0, 607, 896, 512) && flags_are(m, 1, 1, 0, 0));
  // the same count: nothing happens, flags included
  EXPECT(m.set_view(5, &err) == 0 && m.set_view(-1, &err) == 0 && flags_are(m, 1, 1, 0, 0) && sizes_are(m, 5, 0, 607, 896, 512));
  // another count drops them; the whole matrix may come into view though its tail is not factored
  EXPECT(m.set_view(3, &err) == 0 && sizes_are(m, 3, 2, 428, 512, 512) && flags_are(m, 0, 0, 0, 0));
  m.weights_resident();
  m.residual_resident();
  EXPECT(m.set_view(3, &err) == 0 && flags_are(m, 1, 1, 0, 0));
  EXPECT(m.set_view(1, &err) == 0 && sizes_are(m, 1, 4, 100, 128, 128) && flags_are(m, 0, 0, 0, 0) && m.pn_fact_all == 512);
  // lpgp_mat_clone from a source that is itself a view
  MatState c;
  EXPECT(c.adopt_prefix(m, 2, &err) == 0);
  EXPECT(sizes_are(c, 2, 0, 228, 256, 256) && flags_are(c, 0, 0, 0, 0) && c.fully_factored());
  EXPECT(block_is(c.blocks[0], 100, 0, 0, 128) && block_is(c.blocks[1], 128, 100, 128, 128));
  EXPECT(sizes_are(m, 1, 4, 100, 128, 128));     // the source is as it was
  MatState d;
  EXPECT(d.adopt_prefix(m, 4, &err) == -2 && err == "lpgp_mat_clone: block 3 is not factored yet");
  EXPECT(d.adopt_prefix(m, 5, &err) == -2 && err == "lpgp_mat_clone: block 4 is not factored yet");     // (no exception for the whole matrix here)
  EXPECT(d.adopt_prefix(m, 0, &err) == -2 && err == "lpgp_mat_clone: 0 of 5 blocks");
  EXPECT(d.adopt_prefix(m, 6, &err) == -2 && err == "lpgp_mat_clone: 6 of 5 blocks");
  EXPECT(sizes_are(d, 0, 0, 0, 0, 0));
  EXPECT(d.adopt_prefix(m, 3, &err) == 0 && sizes_are(d, 3, 0, 428, 512, 512));
  // lpgp_mat_inverse: the blocks in view, not factored
  EXPECT(m.set_view(2, &err) == 0);
  MatState inv;
  inv.adopt_layout(m);
  EXPECT(sizes_are(inv, 2, 0, 228, 256, 0) && block_is(inv.blocks[1], 128, 100, 128, 128) && flags_are(inv, 0, 0, 0, 0));
  // an empty table has no view
  MatState e;
  EXPECT(e.set_view(-1, &err) == -2 && err == "lpgp_mat_set_view: 0 of 0 blocks");
}

static void check_rollback() {
  std::string err;
  MatState m = with_blocks({129});
  m.factored(0);
  m.weights_resident();
  EXPECT(m.push_block(77) == 1 && sizes_are(m, 2, 0, 206, 384, 256));
  m.weights_resident();
  m.residual_resident();
  EXPECT(m.can_pop_block(&err) == 0 && sizes_are(m, 2, 0, 206, 384, 256));
  EXPECT(m.pop_block(&err) == 0 && sizes_are(m, 1, 0, 129, 256, 256) && flags_are(m, 0, 0, 0, 0));
  m.weights_resident();
  EXPECT(m.pop_block(&err) == -2 && err == "lpgp_mat_pop_block: the last block is part of the factor");
  EXPECT(m.can_pop_block(&err) == -2 && sizes_are(m, 1, 0, 129, 256, 256) && flags_are(m, 1, 0, 0, 0));
  MatState e;
  EXPECT(e.pop_block(&err) == -2 && err == "lpgp_mat_pop_block: no block");
  m.push_block(4);
  m.factored(0);
  EXPECT(m.set_view(1, &err) == 0);
  EXPECT(m.pop_block(&err) == -2 && err == "lpgp_mat_pop_block: a strict prefix of the blocks is in view" && sizes_are(m, 1, 1, 129, 256, 256));
  EXPECT(m.pop_block(nullptr) == -2);            // the text is optional
  // a block whose factorisation failed eagerly (status != 0: pn_fact unchanged) can go
  MatState f = with_blocks({128, 1});
  f.factored(129);
  EXPECT(f.pop_block(&err) == 0 && f.pop_block(&err) == 0 && sizes_are(f, 0, 0, 0, 0, 0));
}

int main() {
  static_assert(MatState::TB == 128, "the tile edge");
  check_layout();
  check_enqueue_and_predict();
  check_check();
  check_views();
  check_rollback();
  if (failures) {
    std::printf("mat_state_check: %d checks failed\n", failures);
    return 1;
  }
  std::printf("mat_state_check: all checks passed\n");
  return 0;
}
