// Stand-alone host check of csrc/pivchol_state.h (tests/test_pivchol_host.py builds it with AddressSanitizer + UBSan and runs it):
// the loop pivot -> row pieces -> commit -> finish walked through tilings in every order, gaps, overlaps, pieces out of range, a
// commit without a pivot, use after finish, the stop rules and the borrowers of the factor.  Every refusal must leave the state
// exactly as it was.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "pivchol_state.h"

using lpgp::PivcholState;

static int failures = 0;

static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  if (ok) return;
  ++failures;
  std::printf("pivchol_state_check: %s (%lld, %lld)\n", what, a, b);
}

static bool same(const PivcholState& a, const PivcholState& b) {
  return a.n == b.n && a.max_rank == b.max_rank && a.rank == b.rank && a.rtol == b.rtol && a.d0 == b.d0 && a.pending == b.pending && a.pivot == b.pivot &&
         a.pivot_value == b.pivot_value && a.finished == b.finished && a.delta == b.delta && a.borrowers == b.borrowers && a.pivots == b.pivots &&
         a.pieces == b.pieces;
}

// a transition that must refuse: -2, a text, the state untouched
template <class F>
static void refuses(PivcholState& s, F&& f, const char* what) {
  const PivcholState before = s;
  std::string err;
  const int rc = f(s, &err);
  expect(rc == -2, what, rc);
  expect(!err.empty(), what, -1);
  expect(same(s, before), what, -2);
}

static PivcholState fresh(int64_t n, int32_t rank, double rtol = 1e-6, double d0 = 2.0) {
  PivcholState s;
  s.init(n, rank, rtol, d0);
  return s;
}

using Pieces = std::vector<std::pair<int64_t, int64_t>>;   // (col_off, len)

// one row: the pieces go in (all accepted), the commit succeeds iff they tile [0, n)
static void row_of(int64_t n, const Pieces& pieces, bool tiles) {
  PivcholState s = fresh(n, 3);
  std::string err;
  expect(s.can_pivot(&err) == 0, "can_pivot on a fresh state");
  expect(s.pivot_read(n / 2, 1.5) == n / 2, "pivot taken");
  for (const auto& p : pieces) expect(s.add_piece(p.first, p.second, &err) == 0, "piece accepted", p.first, p.second);
  expect(s.tiled() == tiles, "tiled()", (long long)pieces.size(), tiles);
  if (tiles) {
    expect(s.committed(&err) == 0, "commit of a tiled row");
    expect(s.rank == 1 && s.pending == 0 && s.pivot == -1 && s.pieces.empty(), "state after a commit", s.rank);
    expect(s.pivots.size() == 1 && s.pivots[0] == n / 2, "pivot recorded");
  } else {
    refuses(s, [](PivcholState& t, std::string* e) { return t.committed(e); }, "commit of a row with a gap");
    expect(s.rank == 0 && s.pending == 1, "a refused commit keeps the pivot pending");
    // asking for the pivot again starts the row afresh
    expect(s.pivot_read(n / 2, 1.5) == n / 2 && s.pieces.empty(), "pivot again drops the pieces");
    expect(s.add_piece(0, n, &err) == 0 && s.committed(&err) == 0 && s.rank == 1, "whole row after the refusal");
  }
}

static void tilings() {
  row_of(1, {{0, 1}}, true);
  row_of(201, {{0, 70}, {70, 130}, {200, 1}}, true);
  row_of(201, {{200, 1}, {0, 70}, {70, 130}}, true);            // any order
  row_of(201, {{70, 130}, {0, 0}, {200, 1}, {0, 70}, {201, 0}}, true);   // empty pieces are no pieces (an empty block)
  row_of(201, {{0, 70}, {200, 1}}, false);                       // a gap in the middle
  row_of(201, {{70, 130}, {200, 1}}, false);                     // ... at the start
  row_of(201, {{0, 70}, {70, 130}}, false);                      // ... at the end
  row_of(201, {}, false);                                        // no piece at all
  row_of(5, {{0, 0}}, false);
}

static void refused_pieces() {
  const int64_t big = std::numeric_limits<int64_t>::max();
  PivcholState s = fresh(201, 3);
  // no pivot pending
  refuses(s, [](PivcholState& t, std::string* e) { return t.add_piece(0, 70, e); }, "piece without a pivot");
  refuses(s, [](PivcholState& t, std::string* e) { return t.committed(e); }, "commit without a pivot");
  s.pivot_read(7, 1.0);
  std::string err;
  expect(s.add_piece(0, 70, &err) == 0, "first piece");
  const std::pair<int64_t, int64_t> bad[] = {{-1, 5}, {0, -1}, {200, 2}, {201, 1}, {202, 0}, {150, 52}, {0, 202}, {1, big}, {big, 1}, {big, big}, {-big, 3}};
  for (const auto& p : bad) {
    const PivcholState before = s;
    err.clear();
    expect(s.add_piece(p.first, p.second, &err) == -2 && !err.empty() && same(s, before), "piece out of range", p.first, p.second);
  }
  const std::pair<int64_t, int64_t> over[] = {{0, 70}, {69, 1}, {0, 1}, {10, 20}, {69, 10}, {0, 201}};
  for (const auto& p : over) {
    const PivcholState before = s;
    err.clear();
    expect(s.add_piece(p.first, p.second, &err) == -2 && !err.empty() && same(s, before), "overlapping piece", p.first, p.second);
  }
  expect(s.add_piece(70, 130, &err) == 0 && s.add_piece(200, 1, &err) == 0, "the rest of the row");
  const PivcholState before = s;
  expect(s.add_piece(200, 1, &err) == -2 && same(s, before), "the last piece twice");
  expect(s.committed(&err) == 0 && s.rank == 1, "commit after refused pieces");
}

static void stop_rules() {
  // rank reached
  PivcholState s = fresh(10, 2, 1e-6, 2.0);
  std::string err;
  for (int k = 0; k < 2; ++k) {
    expect(s.pivot_read(k, 1.0) == k, "pivot before the rank is reached", k);
    expect(s.add_piece(0, 10, &err) == 0 && s.committed(&err) == 0, "commit", k);
  }
  expect(s.pivot_read(5, 1.0) == -1 && s.pending == 0 && s.pivot_value == 1.0, "max_rank reached: no pivot, the value kept");
  refuses(s, [](PivcholState& t, std::string* e) { return t.add_piece(0, 10, e); }, "piece after the stop");
  refuses(s, [](PivcholState& t, std::string* e) { return t.committed(e); }, "commit after the stop");
  // n reached (rank asked for above n)
  PivcholState t = fresh(2, 7);
  expect(t.max_rank == 2, "room for min(rank, n) rows", t.max_rank);
  for (int k = 0; k < 2; ++k) {
    expect(t.pivot_read(k, 1.0) == k && t.add_piece(0, 2, &err) == 0 && t.committed(&err) == 0, "commit", k);
  }
  expect(t.pivot_read(0, 1.0) == -1, "n reached");
  // rank 0
  PivcholState z = fresh(4, 0);
  expect(z.pivot_read(1, 2.0) == -1 && !z.pending, "max_rank 0");
  // the rtol stop: value <= rtol * d0 stops, the next double above does not
  PivcholState r = fresh(4, 4, 0.25, 2.0);
  expect(r.pivot_read(1, 0.5) == -1, "value == rtol * d0 stops");
  expect(r.pivot_read(1, 0.25) == -1, "value below rtol * d0 stops");
  expect(r.pivot_read(1, 0.5000000000000001) == 1 && r.pending == 1, "the next double above does not");
  expect(r.pivot_read(1, 0.0) == -1 && r.pending == 0 && r.pieces.empty(), "a stop clears the pending pivot");
}

static void after_finish_and_borrowers() {
  PivcholState s = fresh(3, 3);
  std::string err;
  refuses(s, [](PivcholState& t, std::string* e) { return t.borrow(e); }, "borrow before finish");
  s.pivot_read(2, 1.0);
  expect(s.add_piece(0, 3, &err) == 0 && s.committed(&err) == 0, "one row");
  s.pivot_read(1, 0.5);
  expect(s.add_piece(0, 2, &err) == 0, "a piece of the second row");
  expect(s.finish(0.125, &err) == 0, "finish with a pivot pending");
  expect(s.finished == 1 && s.delta == 0.125 && s.pending == 0 && s.pivot == -1 && s.pieces.empty() && s.rank == 1, "state after finish", s.rank);
  refuses(s, [](PivcholState& t, std::string* e) { return t.can_pivot(e); }, "pivot after finish");
  refuses(s, [](PivcholState& t, std::string* e) { return t.add_piece(0, 3, e); }, "piece after finish");
  refuses(s, [](PivcholState& t, std::string* e) { return t.committed(e); }, "commit after finish");
  refuses(s, [](PivcholState& t, std::string* e) { return t.finish(1.0, e); }, "finish twice");
  expect(s.can_destroy(&err) == 0, "destroy without borrowers");
  expect(s.borrow(&err) == 0 && s.borrow(&err) == 0 && s.borrowers == 2, "two borrowers", s.borrowers);
  refuses(s, [](PivcholState& t, std::string* e) { return t.can_destroy(e); }, "destroy while borrowed");
  s.give_back();
  refuses(s, [](PivcholState& t, std::string* e) { return t.can_destroy(e); }, "destroy while one borrower is left");
  s.give_back();
  expect(s.can_destroy(&err) == 0 && s.borrowers == 0, "destroy after both gave back");
  s.give_back();
  expect(s.borrowers == 0, "give_back below zero");
}

int main() {
  tilings();
  refused_pieces();
  stop_rules();
  after_finish_and_borrowers();
  if (failures) {
    std::printf("pivchol_state_check: %d check(s) FAILED\n", failures);
    return 1;
  }
  std::printf("pivchol_state_check: all checks passed\n");
  return 0;
}
