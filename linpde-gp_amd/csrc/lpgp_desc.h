// HIP-free part of the internal declarations: error reporting, the lowered kernel descriptor and its
// host-side lowering.  Included by lpgp_internal.h (device build) and by the host-only sources
// (lower.cpp, hosttest/) that are also compiled with the host compiler + AddressSanitizer.
#pragma once

#include <cstdint>

#include "lpgp.h"

namespace lpgp {

constexpr int TILE = 128;          // base tile: potrf_tile block, GEMM block tile, padding unit

void set_error(const char* fmt, ...);
const char* last_error();

#define LPGP_CHECK(cond, ...)                                                       \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      ::lpgp::set_error(__VA_ARGS__);                                               \
      return -2;                                                                    \
    }                                                                               \
  } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// ---- lowered kernel descriptor (device form) ------------------------------------------
// entry = sum_g scale_g * exp(-sum_d E_d(r_d)) * sum_c sgn^{parity_c} Poly_c(r_1..r_d),
// r_d = |a_d (x_d - x'_d)|, E = r (Matern) or r^2/2 (ExpQuad); Poly_c dense nested-Horner
// coefficient tensor.  Built on the host by lower_kdesc (lower.cpp).  A Wendland dimension (expkind 3) replaces its exponential
// by (1 - r_d)_+^{pow_d}: an integer power inside the support, a select of exactly 0.0 outside.
constexpr int MAXCLS = 16;         // parity classes (2^d, d <= 4)
constexpr int RAD_M = 5;           // radial Matern group: psi^(0) .. psi^(4)
constexpr int RAD_NEG = 3;         // ... negative powers of s a Theta_m may carry (p >= 2, m <= 4: at most s^-3)
constexpr int MAXCOEF = 8192;      // coefficient doubles over all groups (only the used part is staged to the device)

struct DevGroup {
  double scale;
  double a[LPGP_MAXD];
  int32_t expkind[LPGP_MAXD];      // 1: exp(-r), 2: exp(-r^2/2); low byte 3: (1 - r)_+^pow (Wendland; the COMPACT instantiations only) with the
                                   // integer power in the bits above it -- ek_kind / ek_pow below.  (The power shares the word because the size of
                                   // this struct and the bytes of every descriptor without a Wendland group are pinned: tests/golden/lowering_c1_c3.npz.)
  int32_t deg[LPGP_MAXD];          // polynomial degree per dim
  int32_t ncls;
  int32_t parity[MAXCLS];          // bit d set => factor sign(x_d - x'_d)
  int32_t coef_off[MAXCLS];        // offset into coef[]
  // isotropic Matern group (LPGP_MATERN_ISO): with u = a .* (x - x'), s = |u|,
  //   entry = scale * exp(-s) * [ Q0(s) + (w . u) Q1(s) + (u^T B u) Q2(s) ],
  // Q0, Q1, Q2 of degree deg[0] at coef_off[0..2] (ncls = 3; parity[0] = 0 so that the constant
  // coefficient of Q0 is the diagonal value, as for the product form)
  // radial Matern group (LPGP_MATERN_RADIAL, iso == 2): up to two derivatives per argument,
  //   entry = scale * exp(-s) * sum_{m=0..4} Theta_m(s) Pi_m(u),   exp(-s) Theta_m(s) = psi^(m)(s^2 / 2),  psi(s^2 / 2) = kappa(s).
  // coef_off[0]: one double, the diagonal value before the scale (ncls = 1, parity[0] = 0: desc_diag reads it like a
  //   product-form class), then Theta_0..Theta_4, rad_theta_len(p) doubles each: the coefficients of s^0..s^p (p = deg[0]), then
  //   those of s^-1, s^-2, s^-3 (zero while m <= p).
  // coef_off[1]: the monomials of Pi_0, Pi_1, .., Pi_4 one after another, parity[1 + m] of them for Pi_m, two doubles each: the
  //   coefficient, and a double whose low 32 bits hold the exponents of u_0..u_3, three bits each (a sparse list: 6 monomials
  //   for a pair of Laplacians in 2-D, 15 in 4-D, against 5^d coefficients per m of a dense tensor).
  // isotropic Wendland group (LPGP_WENDLAND_ISO): iso == 1 with expkind[.] == 3, the same three polynomials and
  //   entry = scale * (1 - s)_+^{ek_pow(expkind[0])} * [ Q0(s) + (w . u) Q1(s) + (u^T B u) Q2(s) ]   (inside: s^2 <= 1)
  int32_t iso, has_lin, has_quad;
  double w[LPGP_MAXD];
  double B[LPGP_MAXD * LPGP_MAXD];
};

// DevGroup::expkind of a Wendland dimension: kind 3 and the integer power of (1 - r) the group multiplies by (>= 1 for a product-form
// dimension, >= 0 for an isotropic group, which carries it in every dimension)
constexpr int EK_COMPACT = 3;
constexpr int32_t ek_compact(int pow) { return (int32_t)(EK_COMPACT | (pow << 8)); }
constexpr int ek_kind(int32_t e) { return e & 0xff; }
constexpr int ek_pow(int32_t e) { return e >> 8; }

struct DevDesc {
  int32_t d;
  int32_t ngroups;
  DevGroup g[LPGP_MAXG];
  double coef[MAXCOEF];
};

// doubles of one Theta_m of a radial Matern group (host and device: the lowering writes, eval_entries.h reads by this stride)
constexpr int rad_theta_len(int p) { return p + 1 + RAD_NEG; }
int lower_kdesc(const lpgp_kdesc* kd, int ngroups, DevDesc* out);
// does the lowered descriptor hold a radial Matern group (iso == 2)?  Those are evaluated by the RADIAL instantiations only.
bool desc_has_radial(const DevDesc& desc);
// does it hold a Wendland dimension or an isotropic Wendland group (expkind 3)?  Those are evaluated by the COMPACT instantiations only.
bool desc_has_compact(const DevDesc& desc);
// doubles of the coefficient table the descriptor uses (what travels to the device)
int desc_coef_used(const DevDesc& desc);
// The pair list and the weight counts of lpgp_gram_assemble_weighted / lpgp_cross_assemble_weighted (`fn`: the name in the
// message).  WP_RECT: an off-diagonal block, a < A0 and b < A1.  WP_SYM: a diagonal block, b indexes the row weights (A1 is
// ignored) and the list must hold as many pairs (a, b) as (b, a).  WP_CROSS: every b must be 0 (A1 is ignored).  Also: one
// input dimension for all pairs.  0, or an error with its message set.
enum WpairForm { WP_RECT = 0, WP_SYM = 1, WP_CROSS = 2 };
int check_wpairs(const lpgp_wpair* pairs, int npairs, int A0, int A1, WpairForm form, const char* fn);
// value of sum_g (kd[g])(x, x): only the constant coefficient of the all-even parity classes survives
double desc_diag(const DevDesc& desc);

}  // namespace lpgp
