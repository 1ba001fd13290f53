// Stand-alone check of the per-entry evaluation core on SCATTERED points: lower_kdesc (lower.cpp) and eval_entries (eval_entries.h)
// on the HOST, every entry against the high-precision blocks of tests/_entry_reference.py.  Meant to be built with the host
// compiler and -fsanitize=address,undefined, the sanitizer runtimes linked in statically, and run directly:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
//       -I../../include -I.. entries_check.cpp ../lower.cpp
//   ./a.out cases.bin ref.bin K_ENTRY K_ISO_FIRST
// cases.bin (written by tests/test_entry_reference.py), all doubles:
//   ncases, then per case  which K (0: K_ENTRY, 1: K_ISO_FIRST), lower triangle only (0 / 1), d, ngroups,
//   ngroups x (family[d], p[d], lengthscale[d], scale, nterms, nterms x (coef, n0[d], n1[d])), n0, n1, X0[n0 x d], X1[n1 x d]
// ref.bin, all `long double` as NumPy and this compiler lay it out (the test checks that the sizes agree): per case
//   G[n0 x n1], W[n0 x n1], ETA[n0 x n1], ZERO[n0 x n1]
// Every entry must satisfy |got - G| <= K W + ETA (W = sum_g (1 + rho_g) E_g: the envelope weighted by the rounding of the
// exponent's argument; ETA: gradual underflow -- both derived in tests/_entry_reference.py); entries with ZERO != 0 lie beyond the
// clamp of lpgp_exp_neg and must be exactly +-0.  Each case is evaluated four times: through eval_entries<D, 4> (the device's AEK)
// and <D, 8>, plain and through the per-point exponential factors (HostFactors, origin = the strip's first column point; a strip
// with a point further than FACT_TMAX = 32 scaled units from the origin falls back to the plain evaluation, as a device tile
// does).  The descriptor is evaluated from a heap copy of exactly the bytes that travel to the device.  One line per case also
// states the lowered shape (groups, classes, degrees, parities, exponent kinds): the test holds its restatement of the host's
// kernel choice against it.  Exit status 0: everything held.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../eval_entries.h"
#include "host_factors.h"

using namespace lpgp;

static const double kFactTmax = 32.0;       // assemble.hip: FACT_TMAX

template <class T>
static std::vector<T> read_all(const char* path) {
  std::vector<T> buf;
  FILE* f = std::fopen(path, "rb");
  if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  buf.resize((size_t)bytes / sizeof(T));
  if (std::fread(buf.data(), sizeof(T), buf.size(), f) != buf.size()) { std::printf("short read of %s\n", path); std::exit(2); }
  std::fclose(f);
  return buf;
}

// out[n0 x n1]; *nfac / *nplain: strips evaluated with / without the per-point factors (FACT only)
template <int D, int NE, bool FACT>
static void eval_block(const DevDesc* desc, const std::vector<double>& X0, const std::vector<double>& X1, int n0, int n1,
                       std::vector<double>& out, long* nfac, long* nplain) {
  const ExpTab tab{g_exp_table};
  for (int i = 0; i < n0; ++i)
    for (int j0 = 0; j0 < n1; j0 += NE) {
      double dx[D][NE], res[NE];
      HostFactors<D, NE> fac;
      fac.desc = desc;
      for (int k = 0; k < D; ++k) { fac.xr[k] = X0[(size_t)i * D + k]; fac.x0[k] = X1[(size_t)j0 * D + k]; }
      for (int e = 0; e < NE; ++e) {
        const int j = j0 + e < n1 ? j0 + e : n1 - 1;
        for (int k = 0; k < D; ++k) {
          dx[k][e] = X0[(size_t)i * D + k] - X1[(size_t)j * D + k];
          fac.xc[k][e] = X1[(size_t)j * D + k];
        }
      }
      bool use = FACT;
      if (FACT) {
        for (int g = 0; g < desc->ngroups; ++g)
          for (int k = 0; k < D; ++k) {
            if (desc->g[g].iso || desc->g[g].expkind[k] != 1) continue;
            const double a = desc->g[g].a[k];
            if (!(std::fabs(a * (fac.xr[k] - fac.x0[k])) <= kFactTmax)) use = false;
            for (int e = 0; e < NE; ++e)
              if (!(std::fabs(a * (fac.xc[k][e] - fac.x0[k])) <= kFactTmax)) use = false;
          }
      }
      if (use) {
        eval_entries<D, NE, HostFactors<D, NE>>(desc, dx, res, tab, fac);
        ++*nfac;
      } else {
        eval_entries<D, NE>(desc, dx, res, tab);
        ++*nplain;
      }
      for (int e = 0; e < NE && j0 + e < n1; ++e) out[(size_t)i * n1 + j0 + e] = res[e];
    }
}

template <int NE, bool FACT>
static void eval_dim(int d, const DevDesc* desc, const std::vector<double>& X0, const std::vector<double>& X1, int n0, int n1,
                     std::vector<double>& out, long* nfac, long* nplain) {
  switch (d) {
    case 1: eval_block<1, NE, FACT>(desc, X0, X1, n0, n1, out, nfac, nplain); break;
    case 2: eval_block<2, NE, FACT>(desc, X0, X1, n0, n1, out, nfac, nplain); break;
    case 3: eval_block<3, NE, FACT>(desc, X0, X1, n0, n1, out, nfac, nplain); break;
    default: eval_block<4, NE, FACT>(desc, X0, X1, n0, n1, out, nfac, nplain); break;
  }
}

int main(int argc, char** argv) {
  if (argc < 5) {
    std::printf("usage: entries_check cases.bin ref.bin K_ENTRY K_ISO_FIRST\n");
    return 2;
  }
  const std::vector<double> buf = read_all<double>(argv[1]);
  const std::vector<long double> ref = read_all<long double>(argv[2]);
  const long double Ks[2] = {(long double)std::atof(argv[3]), (long double)std::atof(argv[4])};
  const long double eps = std::ldexp(1.0L, -53);
  size_t pos = 0, rpos = 0;
  auto next = [&]() -> double {
    if (pos >= buf.size()) { std::printf("truncated case file\n"); std::exit(2); }
    return buf[pos++];
  };
  const int ncases = (int)next();
  int fail = 0;
  long fac_all = 0, plain_all = 0;
  for (int ci = 0; ci < ncases; ++ci) {
    const int which = (int)next(), lower = (int)next(), d = (int)next(), ng = (int)next();
    if (which < 0 || which > 1 || d < 1 || d > LPGP_MAXD || ng < 1 || ng > LPGP_MAXG) { std::printf("bad case header\n"); return 2; }
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
    std::vector<double> X0((size_t)n0 * d), X1((size_t)n1 * d), got(nn);
    for (auto& v : X0) v = next();
    for (auto& v : X1) v = next();
    if (rpos + 4 * nn > ref.size()) { std::printf("truncated reference file\n"); return 2; }
    const long double *G = ref.data() + rpos, *W = G + nn, *ETA = W + nn, *ZERO = ETA + nn;
    rpos += 4 * nn;
    std::unique_ptr<DevDesc> full(new DevDesc);
    if (lower_kdesc(kd.data(), ng, full.get()) != 0) {
      std::printf("FAIL: case %d does not lower: %s\n", ci, last_error());
      ++fail;
      continue;
    }
    const size_t bytes = offsetof(DevDesc, coef) + (size_t)desc_coef_used(*full) * sizeof(double);
    std::unique_ptr<char[]> raw(new char[bytes]);
    std::memcpy(raw.get(), full.get(), bytes);
    const DevDesc* desc = reinterpret_cast<const DevDesc*>(raw.get());
    const DevGroup& G0 = desc->g[0];
    std::printf("case %d: d=%d groups=%d iso=%d ncls=%d deg=%d,%d,%d,%d parity=%d,%d kinds=%d,%d,%d,%d |", ci, d, desc->ngroups, G0.iso,
                G0.ncls, G0.deg[0], G0.deg[1], G0.deg[2], G0.deg[3], G0.parity[0], G0.ncls > 1 ? G0.parity[1] : 0, G0.expkind[0],
                G0.expkind[1], G0.expkind[2], G0.expkind[3]);
    long nfac = 0, nplain = 0;
    for (int variant = 0; variant < 4; ++variant) {
      long unused_f = 0, unused_p = 0;
      switch (variant) {
        case 0: eval_dim<4, false>(d, desc, X0, X1, n0, n1, got, &unused_f, &unused_p); break;
        case 1: eval_dim<8, false>(d, desc, X0, X1, n0, n1, got, &unused_f, &unused_p); break;
        case 2: eval_dim<4, true>(d, desc, X0, X1, n0, n1, got, &nfac, &nplain); break;
        default: eval_dim<8, true>(d, desc, X0, X1, n0, n1, got, &unused_f, &unused_p); break;
      }
      long double worst = 0.0L;
      long bad = 0, zero_bad = 0;
      for (int i = 0; i < n0; ++i)
        for (int j = 0; j < (lower ? i + 1 : n1) && j < n1; ++j) {
          const size_t q = (size_t)i * n1 + j;
          const long double err = fabsl((long double)got[q] - G[q]);
          if (!(err <= Ks[which] * W[q] + ETA[q])) ++bad;
          const long double over = err > ETA[q] ? err - ETA[q] : 0.0L;
          if (W[q] > 0) worst = fmaxl(worst, over / W[q]);
          if (ZERO[q] != 0.0L && !(got[q] == 0.0)) ++zero_bad;
        }
      std::printf(" %s worst %.3Lf eps (%ld beyond K = %.2Lf eps, %ld beyond the clamp not 0)", variant == 0 ? "ne4" : variant == 1 ? "ne8" : variant == 2 ? "ne4-fact" : "ne8-fact",
                  worst / eps, bad, Ks[which] / eps, zero_bad);
      if (bad || zero_bad) ++fail;
    }
    std::printf(" | strips with factors %ld, without %ld\n", nfac, nplain);
    fac_all += nfac;
    plain_all += nplain;
  }
  if (rpos != ref.size() || pos != buf.size()) { std::printf("FAIL: trailing data in the case files\n"); ++fail; }
  std::printf("strips with factors %ld, without %ld\n", fac_all, plain_all);
  std::printf(fail ? "%d check(s) failed\n" : "entries_check: all checks passed\n", fail);
  return fail ? 1 : 0;
}
