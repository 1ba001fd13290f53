// Stand-alone host check of csrc/mix_table.h (tests/test_mixed_host.py builds it with AddressSanitizer + UBSan and runs it): the
// packing of CSR rows to padded ELL against a literal walk over the rows -- ragged rows, the padding rule (weight 0.0 and the
// row's first index, index 0 for an empty row), S = 1 and S = 32 --, the slot-major image the kernel reads, and the refusals: a row
// width outside 1 .. 32, an index at npts and a negative one (npts - 1 passes), NULL pointers; a refused table is not written.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mix_table.h"

using lpgp::MixTable;

static int failures = 0;

static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  if (ok) return;
  ++failures;
  std::printf("mix_check: %s (%lld, %lld)\n", what, a, b);
}

struct Csr {
  std::vector<int64_t> indptr{0};
  std::vector<int32_t> indices;
  std::vector<double> data;
  void row(const std::vector<int32_t>& cols, double w0) {
    for (size_t k = 0; k < cols.size(); ++k) {
      indices.push_back(cols[k]);
      data.push_back(w0 + 0.25 * (double)k);
    }
    indptr.push_back((int64_t)indices.size());
  }
  int64_t q() const { return (int64_t)indptr.size() - 1; }
};

// pack, build, and hold both to the rows they came from
static void check_pack(const Csr& A, int64_t npts, int32_t want_S) {
  int32_t S = -1;
  std::vector<int32_t> idx;
  std::vector<double> w;
  std::string err;
  int rc = lpgp::mix_pack_csr(A.q(), A.indptr.data(), A.indices.data(), A.data.data(), npts, &S, &idx, &w, &err);
  expect(rc == 0, err.c_str(), rc);
  if (rc != 0) return;
  expect(S == want_S, "row width", S, want_S);
  expect((int64_t)idx.size() == A.q() * S && idx.size() == w.size(), "packed sizes", (long long)idx.size());
  for (int64_t r = 0; r < A.q(); ++r) {
    const int64_t len = A.indptr[(size_t)r + 1] - A.indptr[(size_t)r];
    for (int64_t k = 0; k < S; ++k) {
      const int32_t i = idx[(size_t)(r * S + k)];
      const double v = w[(size_t)(r * S + k)];
      if (k < len) {
        expect(i == A.indices[(size_t)(A.indptr[(size_t)r] + k)] && v == A.data[(size_t)(A.indptr[(size_t)r] + k)], "a stored entry", r, k);
      } else {
        expect(v == 0.0 && i == (len > 0 ? A.indices[(size_t)A.indptr[(size_t)r]] : 0), "the padding rule", r, k);
      }
    }
  }
  MixTable t;
  rc = lpgp::mix_table_build(A.q(), S, idx.data(), w.data(), npts, &t, &err);
  expect(rc == 0, err.c_str(), rc);
  if (rc != 0) return;
  expect(t.q == A.q() && t.S == S && t.npts == npts && (int64_t)t.idx.size() == t.q * S && t.w.size() == t.idx.size(), "table header", t.q, t.S);
  for (int64_t r = 0; r < t.q; ++r)
    for (int32_t s = 0; s < S; ++s)
      expect(t.idx[(size_t)(s * t.q + r)] == idx[(size_t)(r * S + s)] && t.w[(size_t)(s * t.q + r)] == w[(size_t)(r * S + s)], "slot-major image", r, s);
}

static void check_build_refusal(int64_t q, int32_t S, const int32_t* idx, const double* w, int64_t npts, const char* needle) {
  MixTable t;
  t.q = -7;                                      // must stay as it is
  std::string err;
  const int rc = lpgp::mix_table_build(q, S, idx, w, npts, &t, &err);
  expect(rc == -2, "a refusal returns -2", rc);
  expect(err.find(needle) != std::string::npos, needle);
  expect(t.q == -7 && t.idx.empty() && t.w.empty(), "a refused table is not written");
}

static void check_pack_refusal(const Csr& A, int64_t npts, const char* needle) {
  int32_t S = -7;
  std::vector<int32_t> idx;
  std::vector<double> w;
  std::string err;
  const int rc = lpgp::mix_pack_csr(A.q(), A.indptr.data(), A.indices.data(), A.data.data(), npts, &S, &idx, &w, &err);
  expect(rc == -2, "a refusal returns -2", rc);
  expect(err.find(needle) != std::string::npos, needle);
  expect(S == -7 && idx.empty() && w.empty(), "a refused packing writes nothing");
}

int main() {
  static_assert(lpgp::MIX_MAXS == 32, "the row width");
  const int64_t npts = 50;
  {
    // ragged rows with counts 3, 1, 0 (empty), 5, an index at npts - 1
    Csr A;
    A.row({4, 9, 49}, 1.0);
    A.row({7}, -2.0);
    A.row({}, 0.0);
    A.row({0, 1, 2, 3, 49}, 0.5);
    check_pack(A, npts, 5);
  }
  {
    Csr A;                                       // S = 1: one point per row; and a matrix of empty rows alone (S = 1, index 0, weight 0)
    for (int32_t r = 0; r < 50; ++r) A.row({49 - r}, 1.0);
    check_pack(A, npts, 1);
    Csr E;
    E.row({}, 0.0);
    E.row({}, 0.0);
    check_pack(E, npts, 1);
  }
  {
    Csr A;                                       // S = 32, the cap, beside a short row
    std::vector<int32_t> full;
    for (int32_t k = 0; k < 32; ++k) full.push_back(k + 18);
    A.row(full, 3.0);
    A.row({5, 6}, 1.0);
    check_pack(A, npts, 32);
    full.push_back(17);
    Csr B;
    B.row(full, 1.0);
    check_pack_refusal(B, npts, "row 0 has 33 entries, more than 32");
  }
  {
    Csr A;
    A.row({1, 50}, 1.0);
    check_pack_refusal(A, npts, "row 0 names column 50, outside 0 .. 49");
    Csr B;
    B.row({3}, 1.0);
    B.row({-1}, 1.0);
    check_pack_refusal(B, npts, "row 1 names column -1");
    Csr C;
    C.row({3}, 1.0);
    C.indptr[0] = 1;
    check_pack_refusal(C, npts, "indptr does not start at 0");
  }
  {
    const std::vector<int32_t> idx{0, 49, 3, 3};
    const std::vector<double> w{1.0, 2.0, 3.0, 0.0};
    MixTable t;
    std::string err;
    expect(lpgp::mix_table_build(2, 2, idx.data(), w.data(), npts, &t, &err) == 0, "an index at npts - 1 passes");
    std::vector<int32_t> bad = idx;
    bad[1] = 50;
    check_build_refusal(2, 2, bad.data(), w.data(), npts, "idx[0][1] = 50 is outside 0 .. 49");
    bad[1] = -1;
    check_build_refusal(2, 2, bad.data(), w.data(), npts, "idx[0][1] = -1 is outside");
    check_build_refusal(2, 0, idx.data(), w.data(), npts, "S=0 is outside 1 .. 32");
    check_build_refusal(2, 33, idx.data(), w.data(), npts, "S=33 is outside 1 .. 32");
    check_build_refusal(2, 2, nullptr, w.data(), npts, "null argument");
    check_build_refusal(2, 2, idx.data(), nullptr, npts, "null argument");
    check_build_refusal(0, 2, idx.data(), w.data(), npts, "q=0 rows");
  }
  if (failures) {
    std::printf("mix_check: %d checks failed\n", failures);
    return 1;
  }
  std::printf("mix_check: all checks passed\n");
  return 0;
}
