// The host bookkeeping of a pivoted-Cholesky handle (lpgp_pivchol derives from lpgp::PivcholState): where the greedy loop stands --
// how many rows are committed, whether a pivot is pending, which columns of its row have been evaluated, whether the object is
// closed, who borrows the factor.  Every write to these fields is in this file: a transition below is the only writer of the
// fields it names, and the entry points of pivchol.hip put their device work around the calls.  Plain C++17, no HIP:
// csrc/hosttest/pivchol_state_check.cpp walks the transitions on the host.
//
// The loop:  pivot -> (row piece)* -> commit -> pivot -> ... -> finish.  The pieces of one row must tile [0, n) exactly before the
// row can be committed; a piece that leaves [0, n) or overlaps an earlier piece of the same row is refused where it is handed in
// (nothing is launched for it), a gap is refused at the commit.  A new `pivot` call drops the pieces collected so far (the
// remaining diagonal has not changed, so it finds the same pivot).
//
// A transition that can refuse returns 0, or -2 with the refusal in *err (the caller hands the text to set_error unchanged) and
// the state untouched.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace lpgp {

struct PivcholState {
  int64_t n = 0;                   // order of the operator
  int32_t max_rank = 0;            // rows the factor has room for (min(rank asked for, n))
  int32_t rank = 0;                // rows committed
  double rtol = 0.0, d0 = 0.0;     // pivoting stops at a remaining diagonal <= rtol * d0, d0 = max of the diagonal handed in
  int pending = 0;                 // a pivot was read back and its row is not committed yet
  int64_t pivot = -1;              // ... its index
  double pivot_value = 0.0;        // ... and the remaining diagonal there (the RUNNING d[pivot])
  int finished = 0;                // lpgp_pivchol_finish has closed the object: L, delta and the pivots are final
  double delta = 0.0;              // (set by finish)
  int borrowers = 0;               // lpgp_pcg handles that read L in place
  std::vector<int64_t> pivots;     // the committed pivots in their order
  std::vector<std::pair<int64_t, int64_t>> pieces;   // [begin, end) of the row pieces evaluated for the pending pivot

  void init(int64_t n_, int32_t rank_asked, double rtol_, double d0_) {
    n = n_;
    max_rank = (int32_t)std::min<int64_t>(rank_asked, n_);
    rtol = rtol_;
    d0 = d0_;
  }

  // ---- queries -----------------------------------------------------------------------------------------------------------
  bool room() const { return rank < max_rank; }              // (max_rank <= n: "n reached" is the same test)
  // the rule of PivotedCholeskyPreconditioner: a pivot is taken while there is room and its value is above rtol * d0
  bool stops(double value) const { return !room() || value <= rtol * d0; }
  // the pieces of the pending row cover [0, n) exactly once (overlaps never get in: add_piece)
  bool tiled() const {
    std::vector<std::pair<int64_t, int64_t>> s(pieces);
    std::sort(s.begin(), s.end());
    int64_t at = 0;
    for (const auto& p : s) {
      if (p.first != at) return false;
      at = p.second;
    }
    return at == n;
  }

  // ---- the loop ----------------------------------------------------------------------------------------------------------
  int can_pivot(std::string* err) const {
    if (finished) return refuse(err, "lpgp_pivchol_pivot: the factorisation is finished");
    return 0;
  }
  // the argmax came back as (p, value): the pivot is pending unless a stop rule holds.  Returns the pivot handed to the caller (-1: stop)
  int64_t pivot_read(int64_t p, double value) {
    pieces.clear();
    pivot_value = value;
    if (stops(value)) {
      pending = 0;
      pivot = -1;
    } else {
      pending = 1;
      pivot = p;
    }
    return pivot;
  }
  int can_add_piece(int64_t col_off, int64_t len, std::string* err) const {
    if (finished) return refuse(err, "lpgp_pivchol_row: the factorisation is finished");
    if (!pending) return refuse(err, "lpgp_pivchol_row: no pivot pending (lpgp_pivchol_pivot first)");
    if (col_off < 0 || len < 0 || col_off > n || len > n - col_off)
      return refuse(err, "lpgp_pivchol_row: columns [" + std::to_string(col_off) + ", " + std::to_string(col_off) + " + " + std::to_string(len) +
                             ") leave [0, " + std::to_string(n) + ")");
    for (const auto& p : pieces)
      if (len > 0 && col_off < p.second && p.first < col_off + len)
        return refuse(err, "lpgp_pivchol_row: columns [" + std::to_string(col_off) + ", " + std::to_string(col_off + len) + ") overlap the piece [" +
                               std::to_string(p.first) + ", " + std::to_string(p.second) + ") of the same row");
    return 0;
  }
  int add_piece(int64_t col_off, int64_t len, std::string* err) {
    if (const int rc = can_add_piece(col_off, len, err)) return rc;
    if (len > 0) pieces.emplace_back(col_off, col_off + len);
    return 0;
  }
  int can_commit(std::string* err) const {
    if (finished) return refuse(err, "lpgp_pivchol_commit: the factorisation is finished");
    if (!pending) return refuse(err, "lpgp_pivchol_commit: no pivot pending (lpgp_pivchol_pivot first)");
    if (!tiled()) return refuse(err, "lpgp_pivchol_commit: the row pieces do not tile [0, " + std::to_string(n) + ") (a gap)");
    return 0;
  }
  // the row of the pending pivot was written into L[rank]
  int committed(std::string* err) {
    if (const int rc = can_commit(err)) return rc;
    pivots.push_back(pivot);
    ++rank;
    pending = 0;
    pivot = -1;
    pieces.clear();
    return 0;
  }
  int can_finish(std::string* err) const {
    if (finished) return refuse(err, "lpgp_pivchol_finish: the factorisation is finished already");
    return 0;
  }
  // closed with the shift delta; a pending pivot is dropped
  int finish(double delta_, std::string* err) {
    if (const int rc = can_finish(err)) return rc;
    finished = 1;
    delta = delta_;
    pending = 0;
    pivot = -1;
    pieces.clear();
    return 0;
  }

  // ---- borrowers of the factor -------------------------------------------------------------------------------------------
  int borrow(std::string* err) {
    if (!finished) return refuse(err, "lpgp_pcg_create_pivchol: the factorisation is not finished (lpgp_pivchol_finish first)");
    ++borrowers;
    return 0;
  }
  void give_back() {
    if (borrowers > 0) --borrowers;
  }
  int can_destroy(std::string* err) const {
    if (borrowers > 0) return refuse(err, "lpgp_pivchol_destroy: " + std::to_string(borrowers) + " lpgp_pcg handle(s) still borrow the factor");
    return 0;
  }

 private:
  static int refuse(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return -2;
  }
};

}  // namespace lpgp
