// The host bookkeeping of a matrix handle (lpgp_mat derives from lpgp::MatState): the block table -- which observation blocks the
// matrix holds, where each lies in the logical and in the padded order, which of them are in view -- and the factor state -- how
// far the matrix is factored, what is resident beside the factor, whether a status is still owed to the caller.  Every write to
// these fields is in this file: a transition below is the only writer of the fields it names, and the entry points of api.hip put
// their device work around the calls.  Plain C++17, no HIP: csrc/hosttest/mat_state_check.cpp walks the transitions on the host.
//
// A transition that can refuse returns 0, or -2 with the refusal in *err (the caller hands the text to set_error unchanged) and
// the state untouched.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

struct lpgp_block {
  int64_t n;                       // logical rows
  int64_t off;                     // logical offset
  int64_t poff;                    // padded offset (multiple of the tile edge)
  int64_t pn;                      // padded rows
};

namespace lpgp {

struct MatState {
  static constexpr int64_t TB = 128;             // == TILE (lpgp_desc.h)
  std::vector<lpgp_block> blocks;  // blocks of the current VIEW (set_view): a leading run of the observation blocks
  std::vector<lpgp_block> hidden;  // blocks behind the view (appended by later conditionings; their part of the factor stays in place)
  int64_t n = 0;                   // logical size (of the view)
  int64_t pn = 0;                  // padded size in use (of the view)
  int64_t pn_fact = 0;             // padded columns factored so far (of the view)
  int64_t pn_fact_all = 0;         // the same over view + hidden blocks (meaningful while hidden is non-empty)
  int has_w = 0;                   // representer weights resident (lpgp_solve_weights)
  int has_r = 0;                   // residual resident (lpgp_mat_set_residual)
  int unchecked = 0;               // a factorisation was enqueued (lpgp_potrf_enqueue) and its status not read yet
  int status_known = 0;            // lpgp_potrf_predict read the status word back with its results: lpgp_mat_check needs no copy
  int status_value = 0;
  int poisoned = 0;                // a factorisation of this matrix ended undefined -- a hand-over of a resident kernel timed out (device status < 0), or a
                                   // launch failed half way through the in-place factorisation: every entry point that reads or extends the factor fails from then on

  // ---- queries -----------------------------------------------------------------------------------------------------------
  bool fully_factored() const { return pn_fact == pn; }
  int total_blocks() const { return (int)(blocks.size() + hidden.size()); }
  // block i of the view followed by the hidden ones
  const lpgp_block& block_at(int i) const { return (size_t)i < blocks.size() ? blocks[(size_t)i] : hidden[(size_t)i - blocks.size()]; }
  int64_t fact_all() const { return hidden.empty() ? pn_fact : pn_fact_all; }      // padded columns factored over view + hidden
  int64_t padded_end(int nblocks) const { return nblocks > 0 ? block_at(nblocks - 1).poff + block_at(nblocks - 1).pn : 0; }
  // the block whose padded rows hold pivot h (1-based, as a factorisation reports it), over view + hidden; -1: none
  int block_of_pivot(int64_t h) const {
    int found = -1;
    for (int b = 0; b < total_blocks(); ++b)
      if (h - 1 >= block_at(b).poff && h - 1 < block_at(b).poff + block_at(b).pn) found = b;
    return found;
  }
  // the block push_block(n) would add
  lpgp_block next_block(int64_t n_new) const { return lpgp_block{n_new, n, pn, (n_new + TB - 1) / TB * TB}; }

  // ---- the block table ---------------------------------------------------------------------------------------------------
  // a block of n_new rows behind the last one (the whole matrix in view); weights and residual belong to the smaller matrix
  int push_block(int64_t n_new) {
    const lpgp_block b = next_block(n_new);
    blocks.push_back(b);
    n += b.n;
    pn += b.pn;
    has_w = has_r = 0;
    return (int)blocks.size() - 1;
  }
  int can_pop_block(std::string* err) const {
    if (!hidden.empty()) return refuse(err, "lpgp_mat_pop_block: a strict prefix of the blocks is in view");
    if (blocks.empty()) return refuse(err, "lpgp_mat_pop_block: no block");
    if (blocks.back().poff < pn_fact) return refuse(err, "lpgp_mat_pop_block: the last block is part of the factor");
    return 0;
  }
  // the last block, not factored yet, dropped again
  int pop_block(std::string* err) {
    if (const int rc = can_pop_block(err)) return rc;
    n -= blocks.back().n;
    pn -= blocks.back().pn;
    blocks.pop_back();
    has_w = has_r = 0;
    return 0;
  }
  // the leading nblocks blocks of view + hidden can stand alone: the count is in range and the last of them is factored (or,
  // where `whole_ok`, the prefix is everything)
  int can_take_prefix(const char* fn, int nblocks, bool whole_ok, std::string* err) const {
    const int total = total_blocks();
    if (nblocks < 1 || nblocks > total) return refuse(err, std::string(fn) + ": " + std::to_string(nblocks) + " of " + std::to_string(total) + " blocks");
    if (!(whole_ok && nblocks == total) && padded_end(nblocks) > fact_all())
      return refuse(err, std::string(fn) + ": block " + std::to_string(nblocks - 1) + " is not factored yet");
    return 0;
  }
  // the view becomes the leading nblocks blocks (-1: all).  Nothing at all happens when the count is unchanged; otherwise the
  // resident weights / residual belonged to the previous view
  int set_view(int nblocks, std::string* err) {
    if (nblocks < 0) nblocks = total_blocks();
    if (nblocks >= 1 && nblocks == (int)blocks.size()) return 0;
    if (const int rc = can_take_prefix("lpgp_mat_set_view", nblocks, true, err)) return rc;
    const int64_t fa = fact_all();
    const int move = nblocks - (int)blocks.size();
    if (move < 0) {
      hidden.insert(hidden.begin(), blocks.end() + move, blocks.end());
      blocks.resize((size_t)nblocks);
    } else {
      blocks.insert(blocks.end(), hidden.begin(), hidden.begin() + move);
      hidden.erase(hidden.begin(), hidden.begin() + move);
    }
    n = blocks.back().off + blocks.back().n;
    pn = padded_end(nblocks);
    pn_fact_all = fa;
    pn_fact = fa < pn ? fa : pn;
    has_w = has_r = 0;
    return 0;
  }
  // a fresh handle takes the leading nblocks blocks of src (view + hidden), factored: lpgp_mat_clone
  int adopt_prefix(const MatState& src, int nblocks, std::string* err) {
    if (const int rc = src.can_take_prefix("lpgp_mat_clone", nblocks, false, err)) return rc;
    blocks.clear();
    for (int b = 0; b < nblocks; ++b) blocks.push_back(src.block_at(b));
    n = blocks.back().off + blocks.back().n;
    pn = pn_fact = src.padded_end(nblocks);
    return 0;
  }
  // a fresh handle takes the blocks src has in view, not factored (a plain symmetric matrix in the lower triangle): lpgp_mat_inverse
  void adopt_layout(const MatState& src) {
    blocks = src.blocks;
    n = src.n;
    pn = src.pn;
    pn_fact = 0;
  }
  // the blocks from nblocks on dropped (0 <= nblocks <= blocks in view, nothing hidden), whatever an enqueued factorisation made
  // of them: the status flags, the weights and the residual go with them -- `poisoned` stays
  void truncate(int nblocks) {
    blocks.resize((size_t)nblocks);
    n = nblocks ? blocks.back().off + blocks.back().n : 0;
    pn = padded_end(nblocks);
    if (pn_fact > pn) pn_fact = pn;
    unchecked = status_known = 0;
    has_w = has_r = 0;
  }

  // ---- the factor state --------------------------------------------------------------------------------------------------
  // a factorisation that was waited for ended with status h: the factor covers the view only when h == 0 (otherwise pn_fact is unchanged)
  void factored(int h) {
    if (h == 0) pn_fact = pn;
    has_w = has_r = 0;
  }
  // a factorisation was enqueued: the factor covers the view provisionally -- take_status / truncate take it back on failure
  void factor_enqueued(bool keep_residual) {
    pn_fact = pn;
    unchecked = 1;
    status_known = 0;
    has_w = 0;
    if (!keep_residual) has_r = 0;
  }
  void status_stale() { status_known = 0; }        // a read-back of the status word is on its way: a value recorded earlier is void
  void status_read_back(int value) {               // ... and has arrived: worth recording only while a status is owed
    if (!unchecked) return;
    status_value = value;
    status_known = 1;
  }
  void status_pending() {                          // the device word was written behind the library's back (test hook): a status is owed
    unchecked = 1;
    status_known = 0;
  }
  // the owed status h is handed to the caller.  h < 0 is not a pivot: the panel's contents are undefined and the device word
  // stays where it is, so no later pivot failure could be recorded either
  void take_status(int h) {
    unchecked = status_known = 0;
    if (h < 0) poisoned = 1;
  }
  void poison() { poisoned = 1; }
  void weights_resident() { has_w = 1; }
  void residual_resident() { has_r = 1; }
  void storage_moved() { has_r = 0; }              // the residual segment is addressed relative to the capacity, which changed

  // ---- logical (length n) <-> padded (length pn) host vectors of the view ------------------------------------------------
  void scatter_padded(const double* logical, double* padded) const {
    std::memset(padded, 0, (size_t)pn * sizeof(double));
    for (const lpgp_block& b : blocks) std::memcpy(padded + b.poff, logical + b.off, (size_t)b.n * sizeof(double));
  }
  void gather_padded(const double* padded, double* logical) const {
    for (const lpgp_block& b : blocks) std::memcpy(logical + b.off, padded + b.poff, (size_t)b.n * sizeof(double));
  }
  // tab[padded row] = logical row, for the logical rows; the entries of the padding rows are the caller's (a sentinel)
  void logical_of_padded(int32_t* tab) const {
    for (const lpgp_block& b : blocks)
      for (int64_t i = 0; i < b.n; ++i) tab[b.poff + i] = (int32_t)(b.off + i);
  }

 private:
  static int refuse(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return -2;
  }
};

}  // namespace lpgp
