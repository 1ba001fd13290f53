// Host-side lowering of a kernel descriptor (C ABI `lpgp_kdesc`, a term list
//   sum_t c_t prod_d d^{n0} d'^{n1} k_d )
// to the device form `DevDesc`: per parity class a dense polynomial in r_d = |a_d (x_d - x'_d)| with
// exact integer tables for the Matern derivative polynomials (_matern.py:613-639) and the Hermite
// polynomials (_expquad.py).  Pure C++ (no HIP): built into liblpgp.so by hipcc and, with
// -fsanitize=address, into the host-only test library of `build.sh --host-asan`.

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "lpgp_desc.h"

namespace lpgp {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

const char* last_error() { return g_err; }

// ---------------------------------------------------------------------------------------
// host: polynomial tables
// ---------------------------------------------------------------------------------------
static long double ifact(int n) {
  long double r = 1;
  for (int i = 2; i <= n; ++i) r *= i;
  return r;
}

// Integer numerators of P_n for Matern nu = p + 1/2 over the common denominator
// D_p = (2p)!/p!  (c_k D_p = (2p-k)!/((p-k)! k!) 2^k are integers; P_n = P'_{n-1} - P_{n-1}).
static void matern_poly(int p, int n, long double* out /* p+1 */) {
  long double cur[16], nxt[16];
  for (int k = 0; k <= p; ++k)
    cur[k] = ifact(2 * p - k) / (ifact(p - k) * ifact(k)) * std::pow(2.0L, k);
  for (int it = 0; it < n; ++it) {
    for (int k = 0; k <= p; ++k) {
      long double d = (k + 1 <= p) ? (k + 1) * cur[k + 1] : 0.0L;
      nxt[k] = d - cur[k];
    }
    for (int k = 0; k <= p; ++k) cur[k] = nxt[k];
  }
  long double D = ifact(2 * p) / ifact(p);
  // round to double exactly like float(Fraction(num, D)) and continue in long double
  for (int k = 0; k <= p; ++k) out[k] = (long double)(double)(cur[k] / D);
}

// Integer numerators of P_n over D_p = (2p)!/p! (exact in long double for p <= 6, n <= 12).
static long double matern_poly_num(int p, int n, long double* num /* p+1 */) {
  long double cur[16], nxt[16];
  for (int k = 0; k <= p; ++k)
    cur[k] = ifact(2 * p - k) / (ifact(p - k) * ifact(k)) * std::pow(2.0L, k);
  for (int it = 0; it < n; ++it) {
    for (int k = 0; k <= p; ++k) nxt[k] = ((k + 1 <= p) ? (k + 1) * cur[k + 1] : 0.0L) - cur[k];
    for (int k = 0; k <= p; ++k) cur[k] = nxt[k];
  }
  for (int k = 0; k <= p; ++k) num[k] = cur[k];
  return ifact(2 * p) / ifact(p);
}

// Isotropic Matern with at most one derivative per argument (diffops/_matern.py:17-86,138-203):
//   k = kappa(s), s = |u|, u = a .* (x - x');   d/dx_i k = (P_1/s) e^{-s} a_i u_i = -d/dx'_i k
//   d/dx_i d/dx'_j k = -[ a_i a_j u_i u_j (P_2 - P_1/s)/s^2 + a_i^2 delta_ij P_1/s ] e^{-s}
// summed over the term list into  e^{-s} [Q0(s) + (w.u) Q1(s) + (u^T B u) Q2(s)].
static int lower_iso_group(const lpgp_kdesc& K, int d, DevGroup& G, double* coef, int& coef_used) {
  LPGP_CHECK(K.dlog_lengthscale == 0,
             "lower_kdesc: the derivative with respect to a lengthscale is not implemented for the isotropic Matern (LPGP_MATERN_ISO)");
  const int p = K.p[0];
  LPGP_CHECK(p >= 0 && p <= 6, "lower_kdesc: Matern p=%d unsupported", p);
  long double a[LPGP_MAXD];
  for (int j = 0; j < d; ++j) {
    LPGP_CHECK(K.family[j] == LPGP_MATERN_ISO && K.p[j] == p,
               "lower_kdesc: an isotropic Matern spans all dimensions with one nu");
    LPGP_CHECK(K.lengthscale[j] > 0, "lower_kdesc: lengthscale must be positive");
    const double as = std::sqrt(2.0 * (p + 0.5)) / K.lengthscale[j];
    a[j] = as;
    G.a[j] = as;
    G.expkind[j] = 1;
    G.deg[j] = 0;
  }
  G.deg[0] = p;
  G.iso = 1;
  long double c00 = 0, tr = 0, w[LPGP_MAXD] = {0, 0, 0, 0}, B[LPGP_MAXD][LPGP_MAXD] = {};
  bool first = false, second = false;
  for (int t = 0; t < K.nterms; ++t) {
    const lpgp_term& T = K.terms[t];
    int i0 = -1, i1 = -1, o0 = 0, o1 = 0;
    for (int j = 0; j < d; ++j) {
      LPGP_CHECK(T.n0[j] >= 0 && T.n1[j] >= 0, "lower_kdesc: derivative order out of range");
      o0 += T.n0[j];
      o1 += T.n1[j];
      if (T.n0[j]) i0 = j;
      if (T.n1[j]) i1 = j;
    }
    LPGP_CHECK(o0 <= 1 && o1 <= 1,
               "lower_kdesc: the isotropic Matern has closed forms for identity and directional derivatives only");
    if (T.coef == 0.0) continue;
    if (!o0 && !o1) c00 += T.coef;
    else if (o0 && !o1) { w[i0] += T.coef * a[i0]; first = true; }
    else if (!o0 && o1) { w[i1] -= T.coef * a[i1]; first = true; }
    else {
      B[i0][i1] += T.coef * a[i0] * a[i1];
      if (i0 == i1) tr += T.coef * a[i0] * a[i0];
      second = true;
    }
  }
  LPGP_CHECK(!first || p >= 1, "lower_kdesc: Matern-1/2 is not differentiable");
  LPGP_CHECK(!second || p >= 2, "lower_kdesc: a multivariate Matern needs nu >= 5/2 for a derivative on both arguments");
  long double P0[16], P1[16], P2[16];
  const long double D = matern_poly_num(p, 0, P0);
  matern_poly_num(p, 1, P1);
  matern_poly_num(p, 2, P2);
  LPGP_CHECK(coef_used + 3 * (p + 1) <= MAXCOEF, "lower_kdesc: coefficient table overflow");
  double* Q0 = coef + coef_used;
  double* Q1 = Q0 + (p + 1);
  double* Q2 = Q1 + (p + 1);
  for (int k = 0; k <= p; ++k) Q0[k] = Q1[k] = Q2[k] = 0.0;
  // P_1 // s   (P_1(0) = 0 for p >= 1), rounded to double per coefficient like the reference's
  // RationalPolynomial -> np.double conversion
  long double P1s[16] = {0};
  if (p >= 1) for (int k = 0; k < p; ++k) P1s[k] = P1[k + 1];
  for (int k = 0; k <= p; ++k) {
    Q0[k] = (double)(c00 * (long double)(double)(P0[k] / D) - tr * (long double)(double)(P1s[k] / D));
    Q1[k] = (double)(P1s[k] / D);
  }
  if (p >= 2) {
    // -(P_2 - P_1 // s) // s^2   (its two lowest coefficients vanish for p >= 2)
    for (int k = 0; k + 2 <= p; ++k) Q2[k] = -(double)((P2[k + 2] - P1s[k + 2]) / D);
  }
  G.ncls = 3;
  G.parity[0] = 0; G.parity[1] = 1; G.parity[2] = 1;
  G.coef_off[0] = coef_used;
  G.coef_off[1] = coef_used + (p + 1);
  G.coef_off[2] = coef_used + 2 * (p + 1);
  coef_used += 3 * (p + 1);
  G.has_lin = first ? 1 : 0;
  G.has_quad = second ? 1 : 0;
  for (int i = 0; i < LPGP_MAXD; ++i) {
    G.w[i] = (double)w[i];
    // symmetric part only: u^T B u sees nothing else
    for (int j = 0; j < LPGP_MAXD; ++j) G.B[i * LPGP_MAXD + j] = (double)(0.5L * (B[i][j] + B[j][i]));
  }
  return 0;
}

// Isotropic Matern with up to TWO derivatives per argument (LPGP_MATERN_RADIAL).  With u = a .* (x - x'), s = |u|, t = s^2 / 2 and
// psi(t) = kappa(s) the only non-zero derivatives of t are d_i t = u_i and d_i^2 t = 1, so (Faa di Bruno)
//   d_u^alpha psi = sum_{j <= alpha / 2} psi^(|alpha| - |j|)(t) prod_d alpha_d! / (j_d! (alpha_d - 2 j_d)! 2^{j_d}) u_d^{alpha_d - 2 j_d},
//   d/dx_i = a_i d/du_i,  d/dx'_i = -a_i d/du_i,
// and the term list sums into  e^{-s} sum_{m = 0..4} Theta_m(s) Pi_m(u):  e^{-s} Theta_m = psi^(m),  Theta_0 = P_p,
// Theta_{m+1} = (Theta_m' - Theta_m) / s -- a polynomial for m <= p, a finite Laurent polynomial beyond (p = 2: Theta_3 = -1/(3 s),
// Theta_4 = (1 + s)/(3 s^3)); a monomial of Pi_m has degree 2 m - |alpha| >= 2 m - 4, above the most negative power 2 (m - p) - 1
// of Theta_m, so every singular product vanishes at s = 0 and only the constant monomials (m = |alpha| / 2 <= 2 <= p) survive there.
// The Theta_m come from the exact integer numerators over D_p, the monomial coefficients are summed in long double; each is
// rounded to double once.  Layout: lpgp_desc.h.
static int lower_radial_group(const lpgp_kdesc& K, int d, DevGroup& G, double* coef, int& coef_used) {
  LPGP_CHECK(K.dlog_lengthscale == 0,
             "lower_kdesc: the derivative with respect to a lengthscale is not implemented for the isotropic Matern (LPGP_MATERN_RADIAL)");
  const int p = K.p[0];
  LPGP_CHECK(p >= 0 && p <= 6, "lower_kdesc: Matern p=%d unsupported", p);
  long double a[LPGP_MAXD];
  for (int j = 0; j < d; ++j) {
    LPGP_CHECK(K.family[j] == LPGP_MATERN_RADIAL && K.p[j] == p,
               "lower_kdesc: an isotropic Matern spans all dimensions with one nu");
    LPGP_CHECK(K.lengthscale[j] > 0, "lower_kdesc: lengthscale must be positive");
    const double as = std::sqrt(2.0 * (p + 0.5)) / K.lengthscale[j];
    a[j] = as;
    G.a[j] = as;
    G.expkind[j] = 1;
    G.deg[j] = 0;
  }
  G.deg[0] = p;
  G.iso = 2;
  std::map<std::pair<int, int>, long double> mono;          // (m, packed exponents of u) -> coefficient of Pi_m
  bool any = false, high = false;
  for (int t = 0; t < K.nterms; ++t) {
    const lpgp_term& T = K.terms[t];
    int o0 = 0, o1 = 0, al[LPGP_MAXD] = {0, 0, 0, 0};
    for (int j = 0; j < d; ++j) {
      LPGP_CHECK(T.n0[j] >= 0 && T.n1[j] >= 0, "lower_kdesc: derivative order out of range");
      o0 += T.n0[j];
      o1 += T.n1[j];
      al[j] = T.n0[j] + T.n1[j];
    }
    LPGP_CHECK(o0 <= 2 && o1 <= 2,
               "lower_kdesc: the isotropic Matern (LPGP_MATERN_RADIAL) takes at most two derivatives per argument");
    if (T.coef == 0.0) continue;
    any = any || o0 + o1 > 0;
    high = high || o0 == 2 || o1 == 2 || (o0 && o1);
    long double pref = (o1 & 1) ? -(long double)T.coef : (long double)T.coef;
    for (int j = 0; j < d; ++j) pref *= std::pow(a[j], al[j]);
    int jj[LPGP_MAXD] = {0, 0, 0, 0};
    for (;;) {
      long double w = pref;
      int m = o0 + o1, bits = 0;
      for (int j = 0; j < d; ++j) {
        w *= ifact(al[j]) / (ifact(jj[j]) * ifact(al[j] - 2 * jj[j]) * std::pow(2.0L, jj[j]));
        m -= jj[j];
        bits |= (al[j] - 2 * jj[j]) << (3 * j);
      }
      mono[std::make_pair(m, bits)] += w;
      int j = d - 1;
      while (j >= 0) {
        if (2 * (++jj[j]) <= al[j]) break;
        jj[j] = 0;
        --j;
      }
      if (j < 0) break;
    }
  }
  LPGP_CHECK(!any || p >= 1, "lower_kdesc: Matern-1/2 is not differentiable");
  LPGP_CHECK(!high || p >= 2,
             "lower_kdesc: a multivariate Matern needs nu >= 5/2 for two derivatives on one argument or a derivative on both");
  // Theta_m as Laurent polynomials: th[m][OFF + k] = numerator of the coefficient of s^k over D_p
  constexpr int OFF = 12;
  long double th[RAD_M][OFF + 16] = {};
  long double P0[16];
  const long double D = matern_poly_num(p, 0, P0);
  for (int k = 0; k <= p; ++k) th[0][OFF + k] = P0[k];
  for (int m = 0; m + 1 < RAD_M; ++m)
    for (int k = -OFF; k < p; ++k) th[m + 1][OFF + k] = (k + 2) * th[m][OFF + k + 2] - th[m][OFF + k + 1];
  const int TL = rad_theta_len(p);
  int nmono = 0;
  bool used[RAD_M] = {false, false, false, false, false};
  for (auto& kv : mono)
    if (kv.second != 0.0L) {
      ++nmono;
      LPGP_CHECK(kv.first.first >= 0 && kv.first.first < RAD_M, "lower_kdesc: radial order %d out of range", kv.first.first);
      used[kv.first.first] = true;
    }
  const int need = 1 + RAD_M * TL + 2 * nmono;
  LPGP_CHECK(coef_used + need <= MAXCOEF, "lower_kdesc: coefficient table overflow");
  double* base = coef + coef_used;
  double* tab = base + 1;
  for (int m = 0; m < RAD_M; ++m) {
    for (int k = 0; k < TL; ++k) tab[m * TL + k] = 0.0;
    if (!used[m]) continue;                                // (Theta_m of a p below 2 is more singular; nothing reads it)
    for (int k = -OFF; k < -RAD_NEG; ++k)
      LPGP_CHECK(th[m][OFF + k] == 0.0L, "lower_kdesc: the radial Matern table has a power below s^-%d (p=%d)", RAD_NEG, p);
    for (int k = 0; k <= p; ++k) tab[m * TL + k] = (double)(th[m][OFF + k] / D);
    for (int k = 1; k <= RAD_NEG; ++k) tab[m * TL + p + k] = (double)(th[m][OFF - k] / D);
  }
  double* ml = tab + RAD_M * TL;
  int cnt[RAD_M] = {0, 0, 0, 0, 0};
  for (auto& kv : mono) {                                  // (ordered by m, then by the packed exponents)
    if (kv.second == 0.0L) continue;
    const int m = kv.first.first;
    LPGP_CHECK(m <= p || kv.first.second != 0, "lower_kdesc: a singular radial term without a vanishing monomial (p=%d)", p);
    ml[0] = (double)kv.second;
    const unsigned long long bits = (unsigned long long)(unsigned)kv.first.second;
    std::memcpy(ml + 1, &bits, 8);
    ml += 2;
    ++cnt[m];
  }
  // the diagonal value, operation for operation what the evaluation (eval_entries.h: eval_radial_group) computes at u = 0: a
  // constant monomial contributes its coefficient, every other one c * 0; Theta_m(0) is its constant coefficient, the negative
  // powers are switched off
  double tot = 0.0;
  const double* q = tab + RAD_M * TL;
  for (int m = 0; m < RAD_M; ++m) {
    if (cnt[m] == 0) continue;
    double pim = 0.0;
    for (int i = 0; i < cnt[m]; ++i, q += 2) {
      unsigned long long bits;
      std::memcpy(&bits, q + 1, 8);
      pim = std::fma(q[0], bits == 0 ? 1.0 : 0.0, pim);
    }
    tot = std::fma(tab[m * TL], pim, tot);
  }
  base[0] = tot;
  G.ncls = 1;
  G.parity[0] = 0;
  for (int m = 0; m < RAD_M; ++m) G.parity[1 + m] = cnt[m];
  G.coef_off[0] = coef_used;
  G.coef_off[1] = coef_used + 1 + RAD_M * TL;
  coef_used += need;
  return 0;
}

// ---------------------------------------------------------------------------------------
// Wendland's compactly supported functions (Wendland 2004, Def. 9.11, Thm. 9.12-9.13): phi_{d,k} = I^k (1 - r)_+^l,
// l = floor(d / 2) + k + 1, (I f)(r) = int_r^1 t f(t) dt, normalised to phi(0) = 1.  Everything below is exact integer
// arithmetic: W.num is an integer polynomial in r proportional to phi on [0, 1] (content removed), phi = num / num[0].
// With m = l + k,  d^n phi / dr^n = (1 - r)^{m - n} q_n(r),  deg q_n <= k: the division by (1 - r)^{m - n} is synthetic and
// must leave no remainder.  Expanded in powers of r phi has large alternating coefficients (they sum to 11 669 in absolute
// value for d = 4, k = 3); q_0 has positive ones only, which is why the device evaluates the factored form.
// ---------------------------------------------------------------------------------------
typedef __int128 wint;
constexpr int WEND_MAXK = 3;
constexpr int WEND_N = 24;          // coefficients of any polynomial below (degree l + 2 k <= 12 for d <= 4, k <= 3)

static wint wgcd(wint a, wint b) {
  if (a < 0) a = -a;
  if (b < 0) b = -b;
  while (b != 0) { const wint t = a % b; a = b; b = t; }
  return a;
}

struct Wendland {
  int l, k, m, deg;
  wint num[WEND_N];
};

static void wendland_build(int dim, int k, Wendland& W) {
  W.l = dim / 2 + k + 1;
  W.k = k;
  W.m = W.l + k;
  for (int i = 0; i < WEND_N; ++i) W.num[i] = 0;
  // (1 - r)^l
  W.num[0] = 1;
  W.deg = 0;
  for (int it = 0; it < W.l; ++it) {
    for (int i = W.deg + 1; i >= 1; --i) W.num[i] -= W.num[i - 1];
    ++W.deg;
  }
  for (int it = 0; it < k; ++it) {
    // L * int_r^1 t f(t) dt = sum_j c_j (L / (j + 2)) (1 - r^{j + 2}),  L = lcm(2 .. deg + 2)
    wint L = 1;
    for (int j = 2; j <= W.deg + 2; ++j) L = L / wgcd(L, j) * j;
    wint nxt[WEND_N];
    for (int i = 0; i < WEND_N; ++i) nxt[i] = 0;
    for (int j = 0; j <= W.deg; ++j) {
      const wint c = W.num[j] * (L / (j + 2));
      nxt[0] += c;
      nxt[j + 2] -= c;
    }
    W.deg += 2;
    wint g = 0;
    for (int i = 0; i <= W.deg; ++i) g = wgcd(g, nxt[i]);
    for (int i = 0; i < WEND_N; ++i) W.num[i] = g != 0 ? nxt[i] / g : nxt[i];
  }
}

// q (k + 1 + extra integers over the denominator W.num[0]) = (1 - r)^extra * q_n(r),  d^n phi / dr^n = (1 - r)^{m - n} q_n(r);
// n <= m.  false: the division left a remainder (never, by Thm. 9.12: an internal error).
static bool wendland_q(const Wendland& W, int n, int extra, wint* q /* WEND_N */) {
  wint cur[WEND_N];
  int deg = W.deg;
  for (int i = 0; i < WEND_N; ++i) cur[i] = W.num[i];
  for (int it = 0; it < n; ++it) {
    for (int i = 0; i < deg; ++i) cur[i] = (i + 1) * cur[i + 1];
    cur[deg] = 0;
    if (deg > 0) --deg;
  }
  for (int it = 0; it < W.m - n; ++it) {
    // cur = (1 - r) Q:  Q_0 = cur_0, Q_i = cur_i + Q_{i-1}, and cur_deg + Q_{deg-1} = 0
    for (int i = 1; i <= deg; ++i) cur[i] += cur[i - 1];
    if (cur[deg] != 0) return false;
    if (deg > 0) --deg;
  }
  for (int it = 0; it < extra; ++it) {
    for (int i = deg + 1; i >= 1; --i) cur[i] -= cur[i - 1];
    ++deg;
  }
  for (int i = 0; i < WEND_N; ++i) q[i] = cur[i];
  return true;
}

// Isotropic Wendland with at most one derivative per argument: the algebra of lower_iso_group with phi in place of kappa.  With
// u = a .* (x - x'), s = |u|:   d/dx_i phi = a_i u_i phi'/s = -d/dx'_i phi,
//   d/dx_i d/dx'_j phi = -[ a_i a_j u_i u_j (phi'' - phi'/s)/s^2 + a_i^2 delta_ij phi'/s ],
// phi^(n) = (1 - s)^{m - n} q_n(s).  phi'/s is a polynomial times a power of (1 - s) for k >= 1 (q_1(0) = 0) and
// (phi'' - phi'/s)/s^2 for k >= 2 (the odd coefficients of phi below 2 k + 1 vanish); both divisions are checked to be exact.
// With o = the highest total order of a term (0, 1 or 2) the group multiplies by (1 - s)^{m - o} and keeps
//   Q0 = c00 (1 - s)^o q_0 - tr (1 - s)^{o - 1} q_1/s,   Q1 = (1 - s)^{o - 1} q_1/s,   Q2 = -(q_2 - (1 - s) q_1/s)/s^2,
// so a group without derivatives is the factored form (1 - s)^m q_0(s) itself, with the positive coefficients of q_0.
static int lower_wendland_iso_group(const lpgp_kdesc& K, int d, DevGroup& G, double* coef, int& coef_used) {
  LPGP_CHECK(K.dlog_lengthscale == 0,
             "lower_kdesc: the derivative with respect to a lengthscale is not implemented for the Wendland families (LPGP_WENDLAND_ISO)");
  const int k = K.p[0];
  LPGP_CHECK(k >= 0 && k <= WEND_MAXK, "lower_kdesc: Wendland k=%d unsupported (0 .. %d)", k, WEND_MAXK);
  LPGP_CHECK(d >= 2, "lower_kdesc: LPGP_WENDLAND_ISO needs d >= 2 (d = 1 is the product-form family LPGP_WENDLAND)");
  long double a[LPGP_MAXD];
  for (int j = 0; j < d; ++j) {
    LPGP_CHECK(K.family[j] == LPGP_WENDLAND_ISO && K.p[j] == k, "lower_kdesc: an isotropic Wendland spans all dimensions with one k");
    LPGP_CHECK(K.lengthscale[j] > 0, "lower_kdesc: lengthscale must be positive");
    const double as = 1.0 / K.lengthscale[j];
    a[j] = as;
    G.a[j] = as;
    G.deg[j] = 0;
  }
  G.iso = 1;
  long double c00 = 0, tr = 0, w[LPGP_MAXD] = {0, 0, 0, 0}, B[LPGP_MAXD][LPGP_MAXD] = {};
  bool first = false, second = false;
  int omax = 0;
  for (int t = 0; t < K.nterms; ++t) {
    const lpgp_term& T = K.terms[t];
    int i0 = -1, i1 = -1, o0 = 0, o1 = 0;
    for (int j = 0; j < d; ++j) {
      LPGP_CHECK(T.n0[j] >= 0 && T.n1[j] >= 0, "lower_kdesc: derivative order out of range");
      o0 += T.n0[j];
      o1 += T.n1[j];
      if (T.n0[j]) i0 = j;
      if (T.n1[j]) i1 = j;
    }
    LPGP_CHECK(o0 <= 1 && o1 <= 1,
               "lower_kdesc: the isotropic Wendland has closed forms for identity and directional derivatives only");
    LPGP_CHECK(o0 + o1 == 0 || k >= 1, "lower_kdesc: the Wendland function with k = 0 is not differentiable");
    LPGP_CHECK(o0 + o1 < 2 || k >= 2,
               "lower_kdesc: an isotropic Wendland with k = 1 takes no derivative on both arguments (its form carries a 1/s term)");
    if (T.coef == 0.0) continue;
    if (o0 + o1 > omax) omax = o0 + o1;
    if (!o0 && !o1) c00 += T.coef;
    else if (o0 && !o1) { w[i0] += T.coef * a[i0]; first = true; }
    else if (!o0 && o1) { w[i1] -= T.coef * a[i1]; first = true; }
    else {
      B[i0][i1] += T.coef * a[i0] * a[i1];
      if (i0 == i1) tr += T.coef * a[i0] * a[i0];
      second = true;
    }
  }
  Wendland W;
  wendland_build(d, k, W);
  const int o = omax;
  const int deg = k + o;
  wint q0[WEND_N], q1s[WEND_N], q2s[WEND_N], q1s_lo[WEND_N];
  for (int i = 0; i < WEND_N; ++i) q1s[i] = q2s[i] = q1s_lo[i] = 0;
  LPGP_CHECK(wendland_q(W, 0, o, q0), "lower_kdesc: internal error, phi_{%d,%d} is not divisible by its power of (1 - r)", d, k);
  if (o >= 1) {
    wint q1[WEND_N];
    // (1 - s)^{o - 1} q_1 / s
    LPGP_CHECK(wendland_q(W, 1, o - 1, q1) && q1[0] == 0, "lower_kdesc: internal error, phi'_{%d,%d}/s is no polynomial", d, k);
    for (int i = 0; i + 1 < WEND_N; ++i) q1s[i] = q1[i + 1];
  }
  if (o >= 2) {
    wint q1[WEND_N], q2[WEND_N];
    // q_2 - (1 - s) q_1 / s, divided by s^2
    LPGP_CHECK(wendland_q(W, 1, 1, q1) && q1[0] == 0 && wendland_q(W, 2, 0, q2), "lower_kdesc: internal error in the Wendland tables");
    for (int i = 0; i + 1 < WEND_N; ++i) q2[i] -= q1[i + 1];
    LPGP_CHECK(q2[0] == 0 && q2[1] == 0, "lower_kdesc: internal error, (phi'' - phi'/s)/s^2 of phi_{%d,%d} is no polynomial", d, k);
    for (int i = 0; i + 2 < WEND_N; ++i) q2s[i] = -q2[i + 2];
  }
  G.deg[0] = deg;
  for (int j = 0; j < d; ++j) G.expkind[j] = ek_compact(W.m - o);
  LPGP_CHECK(coef_used + 3 * (deg + 1) <= MAXCOEF, "lower_kdesc: coefficient table overflow");
  double* Q0 = coef + coef_used;
  double* Q1 = Q0 + (deg + 1);
  double* Q2 = Q1 + (deg + 1);
  const long double den = (long double)W.num[0];
  for (int i = 0; i <= deg; ++i) {
    Q0[i] = (double)((c00 * (long double)q0[i] - tr * (long double)q1s[i]) / den);
    Q1[i] = (double)((long double)q1s[i] / den);
    Q2[i] = (double)((long double)q2s[i] / den);
  }
  for (int i = deg + 1; i < WEND_N; ++i)
    LPGP_CHECK(q0[i] == 0 && q1s[i] == 0 && q2s[i] == 0, "lower_kdesc: internal error, a Wendland polynomial of degree above %d", deg);
  G.ncls = 3;
  G.parity[0] = 0; G.parity[1] = 1; G.parity[2] = 1;
  G.coef_off[0] = coef_used;
  G.coef_off[1] = coef_used + (deg + 1);
  G.coef_off[2] = coef_used + 2 * (deg + 1);
  coef_used += 3 * (deg + 1);
  G.has_lin = first ? 1 : 0;
  G.has_quad = second ? 1 : 0;
  for (int i = 0; i < LPGP_MAXD; ++i) {
    G.w[i] = (double)w[i];
    for (int j = 0; j < LPGP_MAXD; ++j) G.B[i * LPGP_MAXD + j] = (double)(0.5L * (B[i][j] + B[j][i]));
  }
  return 0;
}

// d / d log lengthscale of one Matern factor of total order n (lpgp_kdesc::dlog_lengthscale).  The factor a^n e^{-r} P_n(r),
// r = a |x - x'|, depends on the lengthscale through a ~ 1 / lengthscale alone, and
//   d/d log a [a^n e^{-r} P_n(r)] = a^n e^{-r} [n P_n(r) + r (P_n' - P_n)(r)] = a^n e^{-r} [n P_n(r) + r P_{n+1}(r)]:
// the same form with one more degree.  out (p + 2 coefficients) = -(n P_n + r P_{n+1}), from the exact integer numerators,
// rounded to double once per coefficient.
static void matern_poly_dlog(int p, int n, long double* out /* p+2 */) {
  long double a[16], b[16];
  const long double D = matern_poly_num(p, n, a);
  matern_poly_num(p, n + 1, b);
  for (int k = 0; k <= p + 1; ++k) {
    const long double num = (k <= p ? n * a[k] : 0.0L) + (k >= 1 ? b[k - 1] : 0.0L);
    out[k] = (long double)(double)(-num / D);
  }
}

// Probabilists' Hermite He_n, ascending coefficients, degree n.
static void hermite_poly(int n, long double* out /* n+1 */) {
  long double a[16] = {1}, b[16];
  int deg = 0;
  for (int it = 0; it < n; ++it) {
    for (int k = 0; k <= deg + 1; ++k) b[k] = 0;
    for (int k = 0; k <= deg; ++k) b[k + 1] += a[k];            // u * He
    for (int k = 1; k <= deg; ++k) b[k - 1] -= k * a[k];        // - He'
    ++deg;
    for (int k = 0; k <= deg; ++k) a[k] = b[k];
  }
  for (int k = 0; k <= n; ++k) out[k] = a[k];
}

// The same for an ExpQuad factor a^n e^{-u^2/2} He_n(u), u = a (x - x'):  d/du [e^{-u^2/2} He_n] = -e^{-u^2/2} He_{n+1}, so
//   d/d log a [a^n e^{-u^2/2} He_n(u)] = a^n e^{-u^2/2} [n He_n(u) - u He_{n+1}(u)]  (parity n, degree n + 2).
// out (n + 3 coefficients) = -(n He_n - u He_{n+1}); integers, exact.
static void hermite_poly_dlog(int n, long double* out /* n+3 */) {
  long double a[16], b[16];
  hermite_poly(n, a);
  hermite_poly(n + 1, b);
  for (int k = 0; k <= n + 2; ++k) out[k] = (k >= 1 ? b[k - 1] : 0.0L) - (k <= n ? n * a[k] : 0.0L);
}

int lower_kdesc(const lpgp_kdesc* kd, int ngroups, DevDesc* out) {
  LPGP_CHECK(kd != nullptr && ngroups >= 1 && ngroups <= LPGP_MAXG, "lower_kdesc: bad ngroups %d", ngroups);
  std::memset(out, 0, offsetof(DevDesc, coef));      // header and groups; the coefficient table (64 KB) is written where it is used
  const int d = kd[0].d;
  LPGP_CHECK(d >= 1 && d <= LPGP_MAXD, "lower_kdesc: d=%d out of range", d);
  out->d = d;
  out->ngroups = ngroups;
  int coef_used = 0;
  for (int g = 0; g < ngroups; ++g) {
    const lpgp_kdesc& K = kd[g];
    LPGP_CHECK(K.d == d, "lower_kdesc: group %d has d=%d != %d", g, K.d, d);
    LPGP_CHECK(K.nterms >= 1 && K.nterms <= LPGP_MAXT, "lower_kdesc: nterms=%d", K.nterms);
    DevGroup& G = out->g[g];
    G.scale = K.scale;
    if (K.family[0] == LPGP_MATERN_ISO) {
      int rc = lower_iso_group(K, d, G, out->coef, coef_used);
      if (rc != 0) return rc;
      continue;
    }
    if (K.family[0] == LPGP_MATERN_RADIAL) {
      int rc = lower_radial_group(K, d, G, out->coef, coef_used);
      if (rc != 0) return rc;
      continue;
    }
    if (K.family[0] == LPGP_WENDLAND_ISO) {
      int rc = lower_wendland_iso_group(K, d, G, out->coef, coef_used);
      if (rc != 0) return rc;
      continue;
    }
    LPGP_CHECK(K.dlog_lengthscale >= 0 && K.dlog_lengthscale <= d, "lower_kdesc: dlog_lengthscale=%d out of range (0 .. d=%d)",
               K.dlog_lengthscale, d);
    const int jd = K.dlog_lengthscale - 1;       // the dimension whose factor is differentiated by its log lengthscale (-1: none)
    long double a[LPGP_MAXD];
    // Wendland dimensions (LPGP_WENDLAND): a term of total order n = n0 + n1 <= 2 k contributes
    //   a^n (-1)^{n1} sign(x - x')^n (1 - r)^{m - n} q_n(r),   r = a |x - x'|, a = 1 / lengthscale, m = l + k = 2 k + 1;
    // the group multiplies by the common power (1 - r)_+^{m - nmax} (nmax: the highest order of the dimension over the terms)
    // and the coefficient tensor keeps (1 - r)^{nmax - n} q_n(r), of degree <= k + nmax <= 9
    Wendland wend[LPGP_MAXD];
    int wmax[LPGP_MAXD] = {0, 0, 0, 0};
    for (int j = 0; j < d; ++j) {
      LPGP_CHECK(K.lengthscale[j] > 0, "lower_kdesc: lengthscale must be positive");
      if (K.family[j] == LPGP_WENDLAND) {
        LPGP_CHECK(K.dlog_lengthscale == 0,
                   "lower_kdesc: the derivative with respect to a lengthscale is not implemented for the Wendland families (LPGP_WENDLAND)");
        LPGP_CHECK(K.p[j] >= 0 && K.p[j] <= WEND_MAXK, "lower_kdesc: Wendland k=%d unsupported (0 .. %d)", K.p[j], WEND_MAXK);
        wendland_build(1, K.p[j], wend[j]);
        for (int t = 0; t < K.nterms; ++t) {
          const int n0 = K.terms[t].n0[j], n1 = K.terms[t].n1[j];
          LPGP_CHECK(n0 >= 0 && n1 >= 0, "lower_kdesc: derivative order out of range");
          LPGP_CHECK(n0 + n1 <= 2 * K.p[j], "lower_kdesc: a Wendland factor with k = %d is not %d times differentiable (at most 2 k)",
                     K.p[j], n0 + n1);
          if (n0 + n1 > wmax[j]) wmax[j] = n0 + n1;
        }
        a[j] = 1.0 / K.lengthscale[j];
        G.expkind[j] = ek_compact(wend[j].m - wmax[j]);
      } else if (K.family[j] == LPGP_MATERN_HALFINT) {
        LPGP_CHECK(K.p[j] >= 0 && K.p[j] <= 6, "lower_kdesc: Matern p=%d unsupported", K.p[j]);
        // probnum Matern._scale_factors = sqrt(2 nu) / lengthscale, in fp64 like the reference
        double as = std::sqrt(2.0 * (K.p[j] + 0.5)) / K.lengthscale[j];
        a[j] = as;
        G.expkind[j] = 1;
      } else if (K.family[j] == LPGP_EXPQUAD) {
        a[j] = 1.0 / K.lengthscale[j];
        G.expkind[j] = 2;
      } else {
        LPGP_CHECK(false, "lower_kdesc: unknown family %d", K.family[j]);
      }
      G.a[j] = (double)a[j];
    }
    // degrees
    for (int j = 0; j < d; ++j) {
      int deg = 0;
      for (int t = 0; t < K.nterms; ++t) {
        int n = K.terms[t].n0[j] + K.terms[t].n1[j];
        LPGP_CHECK(K.terms[t].n0[j] >= 0 && K.terms[t].n1[j] >= 0 && n <= 12,
                   "lower_kdesc: derivative order out of range");
        int dg = (K.family[j] == LPGP_MATERN_HALFINT) ? K.p[j] : n;
        if (K.family[j] == LPGP_WENDLAND) dg = K.p[j] + wmax[j] - n;
        if (j == jd) dg += (K.family[j] == LPGP_MATERN_HALFINT) ? 1 : 2;
        if (dg > deg) deg = dg;
      }
      G.deg[j] = deg;
    }
    int tsize = 1;
    for (int j = 0; j < d; ++j) tsize *= (G.deg[j] + 1);
    // accumulate per parity class
    std::vector<std::vector<long double>> cls(1 << d);
    for (int t = 0; t < K.nterms; ++t) {
      const lpgp_term& T = K.terms[t];
      int parity = 0;
      long double pref = T.coef;
      long double q[LPGP_MAXD][16];
      int qdeg[LPGP_MAXD];
      for (int j = 0; j < d; ++j) {
        int n = T.n0[j] + T.n1[j];
        if (n & 1) parity |= (1 << j);
        pref *= std::pow(a[j], n);
        if (K.family[j] == LPGP_WENDLAND) {
          if (T.n1[j] & 1) pref = -pref;
          wint qi[WEND_N];
          LPGP_CHECK(wendland_q(wend[j], n, wmax[j] - n, qi), "lower_kdesc: internal error, phi_{1,%d}^(%d) is not divisible by its power of (1 - r)",
                     K.p[j], n);
          qdeg[j] = K.p[j] + wmax[j] - n;
          for (int i = 0; i <= qdeg[j]; ++i) q[j][i] = (long double)qi[i] / (long double)wend[j].num[0];
        } else if (K.family[j] == LPGP_MATERN_HALFINT) {
          if (T.n1[j] & 1) pref = -pref;
          if (j == jd) matern_poly_dlog(K.p[j], n, q[j]);
          else matern_poly(K.p[j], n, q[j]);
          qdeg[j] = K.p[j] + (j == jd ? 1 : 0);
        } else {
          if (T.n0[j] & 1) pref = -pref;
          if (j == jd) hermite_poly_dlog(n, q[j]);
          else hermite_poly(n, q[j]);
          qdeg[j] = n + (j == jd ? 2 : 0);
        }
      }
      auto& C = cls[parity];
      if (C.empty()) C.assign(tsize, 0.0L);
      // tensor product of the per-dim polynomials
      int idx[LPGP_MAXD] = {0, 0, 0, 0};
      for (;;) {
        long double v = pref;
        int lin = 0;
        for (int j = 0; j < d; ++j) {
          v *= q[j][idx[j]];
          lin = lin * (G.deg[j] + 1) + idx[j];
        }
        C[lin] += v;
        int j = d - 1;
        while (j >= 0) {
          if (++idx[j] <= qdeg[j]) break;
          idx[j] = 0;
          --j;
        }
        if (j < 0) break;
      }
    }
    G.ncls = 0;
    for (int c = 0; c < (1 << d); ++c) {
      if (cls[c].empty()) continue;
      bool nz = false;
      for (long double v : cls[c]) nz |= (v != 0.0L);
      if (!nz) continue;
      LPGP_CHECK(coef_used + tsize <= MAXCOEF, "lower_kdesc: coefficient table overflow");
      G.parity[G.ncls] = c;
      G.coef_off[G.ncls] = coef_used;
      for (int i = 0; i < tsize; ++i) out->coef[coef_used + i] = (double)cls[c][i];
      coef_used += tsize;
      ++G.ncls;
    }
  }
  return 0;
}

double desc_diag(const DevDesc& desc) {
  double v = 0.0;
  for (int g = 0; g < desc.ngroups; ++g)
    for (int c = 0; c < desc.g[g].ncls; ++c)
      if (desc.g[g].parity[c] == 0) v += desc.g[g].scale * desc.coef[desc.g[g].coef_off[c]];
  return v;
}

bool desc_has_compact(const DevDesc& desc) {
  for (int g = 0; g < desc.ngroups; ++g)
    for (int j = 0; j < desc.d; ++j)
      if (ek_kind(desc.g[g].expkind[j]) == EK_COMPACT) return true;
  return false;
}

bool desc_has_radial(const DevDesc& desc) {
  for (int g = 0; g < desc.ngroups; ++g)
    if (desc.g[g].iso == 2) return true;
  return false;
}

int desc_coef_used(const DevDesc& desc) {
  int ncoef = 0;
  for (int gi = 0; gi < desc.ngroups; ++gi) {
    const DevGroup& G = desc.g[gi];
    if (G.iso == 2) {
      int end = G.coef_off[1];
      for (int m = 0; m < RAD_M; ++m) end += 2 * G.parity[1 + m];
      if (end > ncoef) ncoef = end;
      continue;
    }
    // (product form: a dense tensor per class; the isotropic Matern and Wendland groups: three polynomials of degree deg[0], deg[1..] = 0)
    for (int c = 0; c < G.ncls; ++c) {
      int len = 1;
      for (int dd = 0; dd < desc.d; ++dd) len *= G.deg[dd] + 1;
      if (G.coef_off[c] + len > ncoef) ncoef = G.coef_off[c] + len;
    }
  }
  return ncoef;
}

// ---------------------------------------------------------------------------------------
// pair list of a variable-coefficient block (lpgp_gram_assemble_weighted / lpgp_cross_assemble_weighted)
// ---------------------------------------------------------------------------------------
int check_wpairs(const lpgp_wpair* pairs, int npairs, int A0, int A1, WpairForm form, const char* fn) {
  constexpr int MAXP = LPGP_MAXW * LPGP_MAXW;
  LPGP_CHECK(pairs != nullptr, "%s: null pair list", fn);
  LPGP_CHECK(npairs >= 1 && npairs <= MAXP, "%s: %d pairs (1 .. %d)", fn, npairs, MAXP);
  LPGP_CHECK(A0 >= 1 && A0 <= LPGP_MAXW, "%s: %d row weight functions (1 .. %d)", fn, A0, LPGP_MAXW);
  const bool sym = form == WP_SYM;
  const int nb = form == WP_CROSS ? 1 : (sym ? A0 : A1);
  LPGP_CHECK(nb >= 1 && nb <= LPGP_MAXW, "%s: %d column weight functions (1 .. %d)", fn, nb, LPGP_MAXW);
  int count[LPGP_MAXW][LPGP_MAXW] = {};
  for (int p = 0; p < npairs; ++p) {
    const lpgp_wpair& P = pairs[p];
    LPGP_CHECK(P.kd != nullptr && P.ngroups >= 1 && P.ngroups <= LPGP_MAXG, "%s: pair %d has no descriptor (or ngroups = %d)", fn, p, P.ngroups);
    LPGP_CHECK(P.a >= 0 && P.a < A0, "%s: pair %d: row weight index %d outside 0 .. %d", fn, p, P.a, A0 - 1);
    LPGP_CHECK(P.b >= 0 && P.b < nb, "%s: pair %d: column weight index %d outside 0 .. %d", fn, p, P.b, nb - 1);
    for (int g = 0; g < P.ngroups; ++g)
      LPGP_CHECK(P.kd[g].d == pairs[0].kd[0].d, "%s: pair %d has input dimension %d, pair 0 has %d", fn, p, P.kd[g].d, pairs[0].kd[0].d);
    ++count[P.a][P.b];
  }
  if (sym)
    for (int a = 0; a < A0; ++a)
      for (int b = 0; b < a; ++b)
        LPGP_CHECK(count[a][b] == count[b][a], "%s: the pair list of a diagonal block must be symmetric: %d pair(s) (%d, %d), %d pair(s) (%d, %d)",
                   fn, count[a][b], a, b, count[b][a], b, a);
  return 0;
}

}  // namespace lpgp
