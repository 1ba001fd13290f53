// Host-only TEST library (never loaded by the product): the descriptor lowering of lower.cpp and the
// evaluation core of eval_entries.h compiled with the host compiler + AddressSanitizer
// (`build.sh --host-asan`), so that the non-trivial host C++ of the library -- exact polynomial tables,
// parity-class folding, the isotropic-group folding, descriptor validation -- runs under a sanitizer on
// the CPU box (GPU AddressSanitizer is not available).  tests/test_host_asan.py drives it
// over the descriptor zoo and compares with the oracle.  The option table of options.cpp is in it too
// (tests/test_host_options.py).
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../eval_entries.h"
#include "host_factors.h"
#include "../options.h"

using namespace lpgp;

template <int D>
static void eval_block(const DevDesc& desc, const double* X0, int64_t n0, const double* X1, int64_t n1, double* out) {
  for (int64_t i = 0; i < n0; ++i)
    for (int64_t j0 = 0; j0 < n1; j0 += AE) {
      double dx[D][AE], res[AE];
      for (int e = 0; e < AE; ++e) {
        const int64_t j = (j0 + e < n1) ? j0 + e : n1 - 1;
        for (int dd = 0; dd < D; ++dd) dx[dd][e] = X0[i * D + dd] - X1[j * D + dd];
      }
      eval_entries<D>(&desc, dx, res, ExpTab{g_exp_table});
      for (int e = 0; e < AE && j0 + e < n1; ++e) out[i * n1 + j0 + e] = res[e];
    }
}

// The factored evaluation: HostFactors (host_factors.h) relative to the first column point of the 8-column strip.
template <int D>
static void eval_block_fact(const DevDesc& desc, const double* X0, int64_t n0, const double* X1, int64_t n1, double* out) {
  for (int64_t i = 0; i < n0; ++i)
    for (int64_t j0 = 0; j0 < n1; j0 += AE) {
      double dx[D][AE], res[AE];
      HostFactors<D> fac;
      fac.desc = &desc;
      for (int dd = 0; dd < D; ++dd) { fac.xr[dd] = X0[i * D + dd]; fac.x0[dd] = X1[j0 * D + dd]; }
      for (int e = 0; e < AE; ++e) {
        const int64_t j = (j0 + e < n1) ? j0 + e : n1 - 1;
        for (int dd = 0; dd < D; ++dd) { dx[dd][e] = X0[i * D + dd] - X1[j * D + dd]; fac.xc[dd][e] = X1[j * D + dd]; }
      }
      eval_entries<D, AE, HostFactors<D>>(&desc, dx, res, ExpTab{g_exp_table}, fac);
      for (int e = 0; e < AE && j0 + e < n1; ++e) out[i * n1 + j0 + e] = res[e];
    }
}

extern "C" {

const char* lpgp_host_last_error(void) { return last_error(); }

// out (n0 x n1, C order) = sum_g (kd[g])(X0, X1), X0 / X1 (n x d, C order)
int lpgp_host_kernel_matrix(const lpgp_kdesc* kd, int32_t ngroups, const double* X0, int64_t n0, const double* X1,
                            int64_t n1, double* out) {
  // the descriptor lives on the heap so that AddressSanitizer sees reads past its end
  std::vector<DevDesc> store(1);
  int rc = lower_kdesc(kd, ngroups, &store[0]);
  if (rc != 0) return rc;
  if (n0 <= 0 || n1 <= 0) return 0;
  switch (store[0].d) {
    case 1: eval_block<1>(store[0], X0, n0, X1, n1, out); break;
    case 2: eval_block<2>(store[0], X0, n0, X1, n1, out); break;
    case 3: eval_block<3>(store[0], X0, n0, X1, n1, out); break;
    case 4: eval_block<4>(store[0], X0, n0, X1, n1, out); break;
    default: return -2;
  }
  return 0;
}

// the same block through the factored evaluation path
int lpgp_host_kernel_matrix_fact(const lpgp_kdesc* kd, int32_t ngroups, const double* X0, int64_t n0, const double* X1,
                                 int64_t n1, double* out) {
  std::vector<DevDesc> store(1);
  int rc = lower_kdesc(kd, ngroups, &store[0]);
  if (rc != 0) return rc;
  if (n0 <= 0 || n1 <= 0) return 0;
  switch (store[0].d) {
    case 1: eval_block_fact<1>(store[0], X0, n0, X1, n1, out); break;
    case 2: eval_block_fact<2>(store[0], X0, n0, X1, n1, out); break;
    case 3: eval_block_fact<3>(store[0], X0, n0, X1, n1, out); break;
    case 4: eval_block_fact<4>(store[0], X0, n0, X1, n1, out); break;
    default: return -2;
  }
  return 0;
}

int lpgp_host_kernel_diag(const lpgp_kdesc* kd, int32_t ngroups, double* out_value) {
  std::vector<DevDesc> store(1);
  int rc = lower_kdesc(kd, ngroups, &store[0]);
  if (rc != 0) return rc;
  *out_value = desc_diag(store[0]);
  return 0;
}

// sizeof(lpgp_kdesc) as the C compiler lays it out (the ctypes mirror `_lib.KDesc` must agree)
int64_t lpgp_host_sizeof_kdesc(void) { return (int64_t)sizeof(lpgp_kdesc); }

// The lowered descriptor as bytes: the header and the groups (everything in front of the coefficient table), then the coefficients
// in use.  Returns the number of bytes (written only if they fit into cap), < 0 on a lowering error.
int64_t lpgp_host_lower_bytes(const lpgp_kdesc* kd, int32_t ngroups, unsigned char* out, int64_t cap) {
  std::vector<DevDesc> store(1);
  int rc = lower_kdesc(kd, ngroups, &store[0]);
  if (rc != 0) return rc;
  const DevDesc& d = store[0];
  int64_t used = 0;
  for (int g = 0; g < d.ngroups; ++g) {
    const DevGroup& G = d.g[g];
    int64_t len = 1;
    for (int j = 0; j < d.d; ++j) len *= G.deg[j] + 1;
    if (G.iso) len = G.deg[0] + 1;
    for (int c = 0; c < G.ncls; ++c) used = used > G.coef_off[c] + len ? used : G.coef_off[c] + len;
  }
  const int64_t head = (int64_t)offsetof(DevDesc, coef), total = head + used * (int64_t)sizeof(double);
  if (total <= cap) {
    std::memcpy(out, &d, (size_t)head);
    std::memcpy(out + head, d.coef, (size_t)(used * (int64_t)sizeof(double)));
  }
  return total;
}

// out[i] = lpgp_exp_neg(s[i]): the per-entry exponential of the assembly kernels (eval_entries.h), host instantiation
void lpgp_host_exp_neg(const double* s, int64_t n, double* out) {
  const ExpTab tab{g_exp_table};
  for (int64_t i = 0; i < n; ++i) out[i] = lpgp_exp_neg(s[i], tab);
}

// the option table (options.cpp) on one Options object, as lpgp_init / lpgp_get_option / lpgp_set_option drive it
// (tests/test_host_options.py)
static Options g_options;

void lpgp_host_options_from_env(void) {
  g_options = Options();
  options_from_env(g_options);
}
int lpgp_host_options_get(const char* key, int64_t* value) { return option_get(g_options, key, value); }
int lpgp_host_options_set(const char* key, int64_t value) { return option_set(g_options, key, value); }
int lpgp_host_options_count(void) { return option_count(); }
const char* lpgp_host_options_name(int i) { return option_name(i); }

}  // extern "C"
