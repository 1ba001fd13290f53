// The stencil table of lpgp_mix_create (api.hip) and assemble_mixed_kernel (assemble.hip): row r of an observation block  A @ L  is
//   sum_s w[r][s] * (L u)(x_{idx[r][s]}),   s = 0 .. S - 1,
// in ELL form -- a fixed row width S <= LPGP_MAXS, shorter rows padded with weight 0.0 and the row's first index (an empty row:
// index 0), so that a padded slot reads a point of the set and contributes an exact zero.  Plain C++17, no HIP:
// csrc/hosttest/mix_check.cpp holds the packing, the padding rule and every refusal to their literal formulas on the host.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace lpgp {

constexpr int32_t MIX_MAXS = 32;                 // == LPGP_MAXS (lpgp.h)

// A validated table as the kernel reads it: SLOT-major, entry (r, s) at [s * q + r], so that the 64 lanes of a wave (lane = row)
// read consecutive words.
struct MixTable {
  int64_t q = 0;                                 // rows of the block
  int32_t S = 0;                                 // row width
  int64_t npts = 0;                              // size of the point set the indices refer to
  std::vector<int32_t> idx;                      // S * q
  std::vector<double> w;                         // S * q
};

// idx / w: q x S, C-order (the layout of lpgp_mix_create).  0, or -2 with *err set: a NULL pointer, q < 1, S outside 1 .. MIX_MAXS,
// an index outside 0 .. npts - 1.  *out is written only on success.
inline int mix_table_build(int64_t q, int32_t S, const int32_t* idx, const double* w, int64_t npts, MixTable* out, std::string* err) {
  auto fail = [&](const std::string& msg) {
    if (err) *err = msg;
    return -2;
  };
  if (!idx || !w || !out) return fail("stencil table: null argument");
  if (q < 1 || npts < 1 || npts > (int64_t)INT32_MAX) return fail("stencil table: q=" + std::to_string(q) + " rows over " + std::to_string(npts) + " points");
  if (S < 1 || S > MIX_MAXS) return fail("stencil table: row width S=" + std::to_string(S) + " is outside 1 .. " + std::to_string(MIX_MAXS));
  for (int64_t r = 0; r < q; ++r)
    for (int32_t s = 0; s < S; ++s) {
      const int32_t i = idx[r * S + s];
      if (i < 0 || (int64_t)i >= npts)
        return fail("stencil table: idx[" + std::to_string(r) + "][" + std::to_string(s) + "] = " + std::to_string(i) + " is outside 0 .. " +
                    std::to_string(npts - 1));
    }
  MixTable t;
  t.q = q;
  t.S = S;
  t.npts = npts;
  t.idx.assign((size_t)q * S, 0);
  t.w.assign((size_t)q * S, 0.0);
  for (int64_t r = 0; r < q; ++r)
    for (int32_t s = 0; s < S; ++s) {
      t.idx[(size_t)s * q + r] = idx[r * S + s];
      t.w[(size_t)s * q + r] = w[r * S + s];
    }
  *out = std::move(t);
  return 0;
}

// CSR rows (indptr of q + 1 entries, column indices and values in column order) to the padded q x S C-order arrays
// mix_table_build takes: S = the longest row (at least 1), stored zeros are kept as they are.  0, or -2 with *err set: a NULL
// pointer, an indptr that does not start at 0 or decreases, a row of more than MIX_MAXS entries, a column outside 0 .. npts - 1.
inline int mix_pack_csr(int64_t q, const int64_t* indptr, const int32_t* indices, const double* data, int64_t npts, int32_t* S_out,
                        std::vector<int32_t>* idx_out, std::vector<double>* w_out, std::string* err) {
  auto fail = [&](const std::string& msg) {
    if (err) *err = msg;
    return -2;
  };
  if (!indptr || !S_out || !idx_out || !w_out || q < 1 || npts < 1) return fail("stencil table: bad argument");
  if (indptr[0] != 0) return fail("stencil table: indptr does not start at 0");
  int64_t longest = 1;
  for (int64_t r = 0; r < q; ++r) {
    const int64_t len = indptr[r + 1] - indptr[r];
    if (len < 0) return fail("stencil table: indptr decreases at row " + std::to_string(r));
    if (len > MIX_MAXS)
      return fail("stencil table: row " + std::to_string(r) + " has " + std::to_string(len) + " entries, more than " + std::to_string(MIX_MAXS));
    if (len > longest) longest = len;
  }
  if (indptr[q] > 0 && (!indices || !data)) return fail("stencil table: null argument");
  const int32_t S = (int32_t)longest;
  std::vector<int32_t> idx((size_t)q * S, 0);
  std::vector<double> w((size_t)q * S, 0.0);
  for (int64_t r = 0; r < q; ++r) {
    const int64_t len = indptr[r + 1] - indptr[r];
    for (int64_t k = 0; k < len; ++k) {
      const int32_t c = indices[indptr[r] + k];
      if (c < 0 || (int64_t)c >= npts)
        return fail("stencil table: row " + std::to_string(r) + " names column " + std::to_string(c) + ", outside 0 .. " + std::to_string(npts - 1));
      idx[(size_t)r * S + k] = c;
      w[(size_t)r * S + k] = data[indptr[r] + k];
    }
    const int32_t first = len > 0 ? idx[(size_t)r * S] : 0;
    for (int64_t k = len; k < S; ++k) idx[(size_t)r * S + k] = first;      // (weight 0.0 from the fill)
  }
  *S_out = S;
  *idx_out = std::move(idx);
  *w_out = std::move(w);
  return 0;
}

}  // namespace lpgp
