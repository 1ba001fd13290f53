// Stand-alone check of the radial Matern family (LPGP_MATERN_RADIAL): lower_kdesc (lower.cpp: lower_radial_group) and the
// evaluation core the device kernels run (eval_entries.h: eval_radial_group) on the HOST, against golden blocks.  Meant to be built
// with the host compiler and -fsanitize=address,undefined, the sanitizer runtimes linked in statically (the program then does not
// depend on what else the environment loads before it), and run directly:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
//       -I../../include -I.. radial_check.cpp ../lower.cpp
//   ./a.out cases.bin K
// cases.bin (written by tests/test_iso_radial_host.py from tests/golden/iso_radial.npz), all doubles:
//   ncases, then per case  d, p, lengthscale[d], nterms, nterms x (coef, n0[d], n1[d]), n0, n1, X0[n0 x d], X1[n1 x d], G[n0 x n1], E[n0 x n1]
// Every entry must satisfy |got - G| <= K eps E (eps = 2^-53); entries of coincident points must be finite and equal desc_diag
// exactly.  The lowered descriptor is evaluated from a heap copy of exactly the bytes that travel to the device, so a read
// past the used part of the coefficient table is caught.  Also: the refusals of the lowering.  Exit status 0: everything held.
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
                       std::vector<double>& out) {
  constexpr int NE = 4;
  const ExpTab tab{g_exp_table};
  for (int i = 0; i < n0; ++i)
    for (int j0 = 0; j0 < n1; j0 += NE) {
      double dx[D][NE], res[NE];
      for (int e = 0; e < NE; ++e) {
        const int j = j0 + e < n1 ? j0 + e : n1 - 1;
        for (int k = 0; k < D; ++k) dx[k][e] = X0[(size_t)i * D + k] - X1[(size_t)j * D + k];
      }
      eval_entries_radial<D, NE>(desc, dx, res, tab);
      for (int e = 0; e < NE && j0 + e < n1; ++e) out[(size_t)i * n1 + j0 + e] = res[e];
    }
}

static void fill_family(lpgp_kdesc& kd, int d, int p, int family) {
  kd.d = d;
  kd.scale = 1.0;
  for (int j = 0; j < d; ++j) {
    kd.family[j] = family;
    kd.p[j] = p;
    kd.lengthscale[j] = 0.5 + 0.25 * j;
  }
}

static void check_refusals() {
  std::unique_ptr<lpgp_kdesc> kd(new lpgp_kdesc());
  std::unique_ptr<DevDesc> dd(new DevDesc);
  auto reset = [&](int d, int p) {
    std::memset(kd.get(), 0, sizeof(lpgp_kdesc));
    fill_family(*kd, d, p, LPGP_MATERN_RADIAL);
    kd->nterms = 1;
    kd->terms[0].coef = 1.0;
  };
  reset(2, 1);
  kd->terms[0].n0[0] = 2;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "5/2"), "p = 1 with a second derivative is refused");
  reset(2, 1);
  kd->terms[0].n0[0] = 1;
  kd->terms[0].n1[1] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "p = 1 with a derivative on both arguments is refused");
  reset(2, 1);
  kd->terms[0].n0[1] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) == 0 && desc_has_radial(*dd), "p = 1 with one first derivative lowers");
  reset(3, 3);
  kd->terms[0].n0[0] = 2;
  kd->terms[0].n0[2] = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "at most two"), "three derivatives on one argument are refused");
  reset(2, 2);
  kd->terms[0].n1[0] = 2;
  kd->dlog_lengthscale = 1;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "lengthscale"), "dlog_lengthscale != 0 is refused");
  reset(2, 7);
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0 && std::strstr(last_error(), "unsupported"), "p = 7 is refused");
  reset(2, 2);
  kd->family[1] = LPGP_MATERN_ISO;
  expect(lower_kdesc(kd.get(), 1, dd.get()) != 0, "mixed families are refused");
  // table overflow: radial groups with every pair of operators of order <= 2 in four dimensions (86 monomials each: sixteen of
  // them still fit) behind three product-form groups that fill most of the table (7^4 coefficients each)
  {
    std::vector<lpgp_kdesc> many(LPGP_MAXG);
    std::vector<std::vector<int>> mi;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        for (int c = 0; c < 3; ++c)
          for (int e = 0; e < 3; ++e)
            if (a + b + c + e <= 2) mi.push_back({a, b, c, e});
    for (auto& K : many) {
      std::memset(&K, 0, sizeof(K));
      fill_family(K, 4, 2, LPGP_MATERN_RADIAL);
      K.nterms = 0;
      for (auto& r : mi)
        for (auto& c : mi) {
          lpgp_term& T = K.terms[K.nterms++];
          T.coef = 1.0 + 0.01 * K.nterms;
          for (int j = 0; j < 4; ++j) { T.n0[j] = r[j]; T.n1[j] = c[j]; }
        }
    }
    expect(lower_kdesc(many.data(), 1, dd.get()) == 0, "one full second-order group in 4-D lowers");
    expect(lower_kdesc(many.data(), LPGP_MAXG, dd.get()) == 0, "sixteen full second-order groups in 4-D lower");
    for (int g = 0; g < 3; ++g) {
      std::memset(&many[g], 0, sizeof(lpgp_kdesc));
      fill_family(many[g], 4, 6, LPGP_MATERN_HALFINT);
      many[g].nterms = 1;
      many[g].terms[0].coef = 1.0;
    }
    expect(lower_kdesc(many.data(), LPGP_MAXG, dd.get()) != 0 && std::strstr(last_error(), "overflow"), "coefficient table overflow is refused");
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("usage: radial_check cases.bin K\n");
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
  for (int ci = 0; ci < ncases; ++ci) {
    std::unique_ptr<lpgp_kdesc> kd(new lpgp_kdesc());
    const int d = (int)next(), p = (int)next();
    if (d < 1 || d > LPGP_MAXD) { std::printf("bad d\n"); return 2; }
    kd->d = d;
    kd->scale = 1.0;
    for (int j = 0; j < d; ++j) {
      kd->family[j] = LPGP_MATERN_RADIAL;
      kd->p[j] = p;
      kd->lengthscale[j] = next();
    }
    kd->nterms = (int)next();
    if (kd->nterms < 1 || kd->nterms > LPGP_MAXT) { std::printf("bad nterms\n"); return 2; }
    for (int t = 0; t < kd->nterms; ++t) {
      kd->terms[t].coef = next();
      for (int j = 0; j < d; ++j) kd->terms[t].n0[j] = (int)next();
      for (int j = 0; j < d; ++j) kd->terms[t].n1[j] = (int)next();
    }
    const int n0 = (int)next(), n1 = (int)next();
    std::vector<double> X0((size_t)n0 * d), X1((size_t)n1 * d), G((size_t)n0 * n1), E((size_t)n0 * n1), got((size_t)n0 * n1);
    for (auto& v : X0) v = next();
    for (auto& v : X1) v = next();
    for (auto& v : G) v = next();
    for (auto& v : E) v = next();
    std::unique_ptr<DevDesc> full(new DevDesc);
    if (lower_kdesc(kd.get(), 1, full.get()) != 0) {
      std::printf("FAIL: case %d does not lower: %s\n", ci, last_error());
      ++g_fail;
      continue;
    }
    expect(desc_has_radial(*full), "a radial group is reported by desc_has_radial");
    // exactly the bytes that are staged to the device
    const size_t bytes = offsetof(DevDesc, coef) + (size_t)desc_coef_used(*full) * sizeof(double);
    std::unique_ptr<char[]> raw(new char[bytes]);
    std::memcpy(raw.get(), full.get(), bytes);
    const DevDesc* desc = reinterpret_cast<const DevDesc*>(raw.get());
    switch (d) {
      case 1: eval_block<1>(desc, X0, X1, n0, n1, got); break;
      case 2: eval_block<2>(desc, X0, X1, n0, n1, got); break;
      case 3: eval_block<3>(desc, X0, X1, n0, n1, got); break;
      default: eval_block<4>(desc, X0, X1, n0, n1, got); break;
    }
    const double diag = desc_diag(*full);
    double worst = 0.0;
    int bad = 0, ndiag = 0;
    for (int i = 0; i < n0; ++i)
      for (int j = 0; j < n1; ++j) {
        const size_t q = (size_t)i * n1 + j;
        const double err = std::fabs(got[q] - G[q]);
        if (!(err <= K * eps * E[q])) ++bad;
        if (E[q] > 0) worst = std::fmax(worst, err / (eps * E[q]));
        bool same = true;
        for (int k = 0; k < d; ++k) same = same && X0[(size_t)i * d + k] == X1[(size_t)j * d + k];
        if (same) {
          ++ndiag;
          if (!(std::isfinite(got[q]) && got[q] == diag)) {
            std::printf("FAIL: case %d entry (%d, %d) of coincident points is %.17g, desc_diag says %.17g\n", ci, i, j, got[q], diag);
            ++g_fail;
          }
        }
      }
    std::printf("case %d: d=%d p=%d nterms=%d  worst |err| / (eps E) = %.3f  (%d coincident entries, %d entries over K = %g)\n", ci, d, p,
                kd->nterms, worst, ndiag, bad, K);
    if (bad) ++g_fail;
    worst_all = std::fmax(worst_all, worst);
  }
  check_refusals();
  std::printf("worst over all cases: %.3f\n", worst_all);
  std::printf(g_fail ? "%d check(s) failed\n" : "radial_check: all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
