// Stand-alone check of the Wendland families (LPGP_WENDLAND, LPGP_WENDLAND_ISO): lower_kdesc (lower.cpp) and the COMPACT
// instantiation of the evaluation core the device kernels run (eval_entries.h) on the HOST, against exact blocks.  Meant to be
// built with the host compiler and -fsanitize=address,undefined, the sanitizer runtimes linked in statically, and run directly:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
//       -I../../include -I.. wendland_check.cpp ../lower.cpp
//   ./a.out cases.bin K
// cases.bin (written by tests/test_wendland_host.py from tests/_wendland_reference.py), all doubles:
//   ncases, then per case  d, ngroups, ngroups x (family[d], p[d], lengthscale[d], scale, nterms, nterms x (coef, n0[d], n1[d])),
//   n0, n1, X0[n0 x d], X1[n1 x d], G[n0 x n1], E[n0 x n1], OUT[n0 x n1]
// Every entry must satisfy |got - G| <= K eps E (eps = 2^-53); entries with OUT != 0 (outside every support) must be exactly
// 0.0; entries of coincident points of a one-group case must equal desc_diag exactly.  The decision the kernels skip empty
// tiles by (lpgp_out_of_reach) is run on the bounding boxes of every 16 x 16 sub-block: where it says "out of reach" every
// evaluated entry of the sub-block must be exactly 0.0.  The descriptor is evaluated from a heap copy of exactly the bytes
// that travel to the device.  Also: the refusals of the lowering.  Exit status 0: everything held.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../eval_entries.h"

using namespace lpgp;

static int g_fail = 0;

static void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAIL: %s (last error: %s)\n", what, last_error());
    ++g_fail;
  }
}

template <int D>
static void eval_block(const DevDesc* desc, const std::vector<double>& X0, const std::vector<double>& X1, int n0, int n1,
                       std::vector<double>& out, int* skipped, int* skip_bad) {
  constexpr int NE = 4;
  const ExpTab tab{g_exp_table};
  for (int i = 0; i < n0; ++i)
    for (int j0 = 0; j0 < n1; j0 += NE) {
      double dx[D][NE], res[NE];
      for (int e = 0; e < NE; ++e) {
        const int j = j0 + e < n1 ? j0 + e : n1 - 1;
        for (int k = 0; k < D; ++k) dx[k][e] = X0[(size_t)i * D + k] - X1[(size_t)j * D + k];
      }
      eval_entries_compact<D, NE>(desc, dx, res, tab);
      for (int e = 0; e < NE && j0 + e < n1; ++e) out[(size_t)i * n1 + j0 + e] = res[e];
    }
  constexpr int SB = 16;
  for (int i0 = 0; i0 < n0; i0 += SB)
    for (int j0 = 0; j0 < n1; j0 += SB) {
      double rlo[D], rhi[D], clo[D], chi[D];
      for (int k = 0; k < D; ++k) { rlo[k] = clo[k] = HUGE_VAL; rhi[k] = chi[k] = -HUGE_VAL; }
      for (int i = i0; i < n0 && i < i0 + SB; ++i)
        for (int k = 0; k < D; ++k) { rlo[k] = std::fmin(rlo[k], X0[(size_t)i * D + k]); rhi[k] = std::fmax(rhi[k], X0[(size_t)i * D + k]); }
      for (int j = j0; j < n1 && j < j0 + SB; ++j)
        for (int k = 0; k < D; ++k) { clo[k] = std::fmin(clo[k], X1[(size_t)j * D + k]); chi[k] = std::fmax(chi[k], X1[(size_t)j * D + k]); }
      if (!lpgp_out_of_reach<D>(desc, rlo, rhi, clo, chi)) continue;
      ++*skipped;
      for (int i = i0; i < n0 && i < i0 + SB; ++i)
        for (int j = j0; j < n1 && j < j0 + SB; ++j)
          if (!(out[(size_t)i * n1 + j] == 0.0)) ++*skip_bad;
    }
}

static void check_refusals() {
  std::unique_ptr<lpgp_kdesc> kd(new lpgp_kdesc());
  std::unique_ptr<DevDesc> dd(new DevDesc);
  auto reset = [&](int d, int k, int family) {
    std::memset(kd.get(), 0, sizeof(lpgp_kdesc));
    kd->d = d;
    kd->scale = 1.0;
    for (int j = 0; j < d; ++j) { kd->family[j] = family; kd->p[j] = k; kd->lengthscale[j] = 0.5 + 0.25 * j; }
    kd->nterms = 1;
    kd->terms[0].coef = 1.0;
  };
  // product form
  reset(1, 2, LPGP_WENDLAND);
  kd->terms[0].n0[0] = 3; kd->terms[0].n1[0] = 2;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "differentiable"), "order 5 at k = 2 is refused");
  reset(1, 2, LPGP_WENDLAND);
  kd->terms[0].n0[0] = 2; kd->terms[0].n1[0] = 2;
  expect(lower_kdesc(kd.get(), 1, dd.get()) == 0 && desc_has_compact(*dd) && !desc_has_radial(*dd) && ek_pow(dd->g[0].expkind[0]) == 1, "order 4 at k = 2 lowers, power 1");
  reset(1, 0, LPGP_WENDLAND);
  kd->terms[0].n0[0] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "a derivative at k = 0 is refused");
  reset(1, 4, LPGP_WENDLAND);
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "unsupported"), "k = 4 is refused");
  reset(2, 2, LPGP_WENDLAND);
  kd->dlog_lengthscale = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "lengthscale"), "dlog_lengthscale != 0 is refused (product form)");
  reset(2, 2, LPGP_WENDLAND);
  kd->family[1] = LPGP_MATERN_HALFINT;
  kd->terms[0].n0[1] = 2;
  expect(lower_kdesc(kd.get(), 1, dd.get()) == 0 && desc_has_compact(*dd) && ek_kind(dd->g[0].expkind[0]) == EK_COMPACT && dd->g[0].expkind[1] == 1,
         "a Wendland factor beside a Matern factor lowers");
  reset(2, 2, LPGP_MATERN_HALFINT);
  expect(lower_kdesc(kd.get(), 1, dd.get()) == 0 && !desc_has_compact(*dd), "a Matern product is not compact");
  // isotropic
  reset(2, 2, LPGP_WENDLAND_ISO);
  kd->terms[0].n0[0] = 2;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "directional"), "two derivatives on one argument are refused");
  reset(2, 2, LPGP_WENDLAND_ISO);
  kd->terms[0].n0[0] = 1; kd->terms[0].n0[1] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "two derivatives on one argument over two dimensions are refused");
  reset(3, 0, LPGP_WENDLAND_ISO);
  kd->terms[0].n1[2] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "k = 0"), "a derivative at k = 0 is refused (isotropic)");
  reset(3, 1, LPGP_WENDLAND_ISO);
  kd->terms[0].n0[0] = 1; kd->terms[0].n1[2] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "1/s"), "a derivative on both arguments at k = 1 is refused");
  reset(3, 1, LPGP_WENDLAND_ISO);
  kd->terms[0].n0[0] = 1; kd->terms[0].n1[2] = 1; kd->terms[0].coef = 0.0;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "... also with a zero coefficient: orders are checked before zero terms are dropped");
  reset(3, 1, LPGP_WENDLAND_ISO);
  kd->terms[0].n1[1] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) == 0 && desc_has_compact(*dd) && dd->g[0].iso == 1, "one derivative at k = 1 lowers");
  reset(2, 2, LPGP_WENDLAND_ISO);
  kd->dlog_lengthscale = 2;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "lengthscale"), "dlog_lengthscale != 0 is refused (isotropic)");
  reset(2, 2, LPGP_WENDLAND_ISO);
  kd->family[1] = LPGP_WENDLAND;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "mixed families are refused");
  reset(2, 2, LPGP_WENDLAND);
  kd->family[1] = LPGP_WENDLAND_ISO;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "an isotropic family inside a product is refused");
  reset(1, 2, LPGP_WENDLAND_ISO);
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "LPGP_WENDLAND_ISO with d = 1 is refused");
  reset(4, 4, LPGP_WENDLAND_ISO);
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "unsupported"), "k = 4 is refused (isotropic)");
  reset(2, 2, 7);
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "unknown family"), "family 7 is unknown");
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: wendland_check cases.bin K\n");
    return 2;
  }
  std::vector<double> buf;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    buf.resize((size_t)bytes / 8);
    if (std::fread(buf.data(), 8, buf.size(), f) != buf.size()) { std::printf("short read\n"); return 2; }
    std::fclose(f);
  }
  const double K = std::atof(argv[2]);
  const double eps = std::ldexp(1.0, -53);
  size_t pos = 0;
  auto next = [&]() -> double {
    if (pos >= buf.size()) { std::printf("truncated case file\n"); std::exit(2); }
    return buf[pos++];
  };
  const int ncases = (int)next();
  double worst_all = 0.0;
  int skipped_all = 0;
  for (int ci = 0; ci < ncases; ++ci) {
    const int d = (int)next(), ng = (int)next();
    if (d < 1 || d > LPGP_MAXD || ng < 1 || ng > LPGP_MAXG) { std::printf("bad d / ngroups\n"); return 2; }
    std::vector<lpgp_kdesc> kd((size_t)ng);
    for (int g = 0; g < ng; ++g) {
      std::memset(&kd[g], 0, sizeof(lpgp_kdesc));
      kd[g].d = d;
      for (int j = 0; j < d; ++j) kd[g].family[j] = (int)next();
      for (int j = 0; j < d; ++j) kd[g].p[j] = (int)next();
      for (int j = 0; j < d; ++j) kd[g].lengthscale[j] = next();
      kd[g].scale = next();
      kd[g].nterms = (int)next();
      if (kd[g].nterms < 1 || kd[g].nterms > LPGP_MAXT) { std::printf("bad nterms\n"); return 2; }
      for (int t = 0; t < kd[g].nterms; ++t) {
        kd[g].terms[t].coef = next();
        for (int j = 0; j < d; ++j) kd[g].terms[t].n0[j] = (int)next();
        for (int j = 0; j < d; ++j) kd[g].terms[t].n1[j] = (int)next();
      }
    }
    const int n0 = (int)next(), n1 = (int)next();
    const size_t nn = (size_t)n0 * n1;
    std::vector<double> X0((size_t)n0 * d), X1((size_t)n1 * d), G(nn), E(nn), OUT(nn), got(nn);
    for (auto& v : X0) v = next();
    for (auto& v : X1) v = next();
    for (auto& v : G) v = next();
    for (auto& v : E) v = next();
    for (auto& v : OUT) v = next();
    std::unique_ptr<DevDesc> full(new DevDesc);
    if (lower_kdesc(kd.data(), ng, full.get()) != 0) {
      std::printf("FAIL: case %d does not lower: %s\n", ci, last_error());
      ++g_fail;
      continue;
    }
    expect(desc_has_compact(*full), "a Wendland group is reported by desc_has_compact");
    const size_t bytes = offsetof(DevDesc, coef) + (size_t)desc_coef_used(*full) * sizeof(double);
    std::unique_ptr<char[]> raw(new char[bytes]);
    std::memcpy(raw.get(), full.get(), bytes);
    const DevDesc* desc = reinterpret_cast<const DevDesc*>(raw.get());
    int skipped = 0, skip_bad = 0;
    switch (d) {
      case 1: eval_block<1>(desc, X0, X1, n0, n1, got, &skipped, &skip_bad); break;
      case 2: eval_block<2>(desc, X0, X1, n0, n1, got, &skipped, &skip_bad); break;
      case 3: eval_block<3>(desc, X0, X1, n0, n1, got, &skipped, &skip_bad); break;
      default: eval_block<4>(desc, X0, X1, n0, n1, got, &skipped, &skip_bad); break;
    }
    const double diag = desc_diag(*full);
    double worst = 0.0;
    int bad = 0, ndiag = 0, nout = 0, out_bad = 0;
    for (int i = 0; i < n0; ++i)
      for (int j = 0; j < n1; ++j) {
        const size_t q = (size_t)i * n1 + j;
        const double err = std::fabs(got[q] - G[q]);
        if (!(err <= K * eps * E[q])) ++bad;
        if (E[q] > 0) worst = std::fmax(worst, err / (eps * E[q]));
        if (OUT[q] != 0.0) {
          ++nout;
          if (!(got[q] == 0.0)) ++out_bad;
        }
        bool same = ng == 1;
        for (int k = 0; k < d; ++k) same = same && X0[(size_t)i * d + k] == X1[(size_t)j * d + k];
        if (same) {
          ++ndiag;
          if (!(std::isfinite(got[q]) && got[q] == diag)) {
            std::printf("FAIL: case %d entry (%d, %d) of coincident points is %.17g, desc_diag says %.17g\n", ci, i, j, got[q], diag);
            ++g_fail;
          }
        }
      }
    std::printf("case %d: d=%d groups=%d  worst |err| / (eps E) = %.3f  (%d over K = %g; %d outside, %d of them not 0; %d coincident; "
                "%d sub-blocks out of reach, %d entries of them not 0)\n", ci, d, ng, worst, bad, K, nout, out_bad, ndiag, skipped, skip_bad);
    if (bad || out_bad || skip_bad) ++g_fail;
    worst_all = std::fmax(worst_all, worst);
    skipped_all += skipped;
  }
  check_refusals();
  std::printf("worst over all cases: %.3f; %d sub-blocks out of reach\n", worst_all, skipped_all);
  std::printf(g_fail ? "%d check(s) failed\n" : "wendland_check: all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
