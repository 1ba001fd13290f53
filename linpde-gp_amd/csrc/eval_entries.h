// Evaluation of one lowered kernel descriptor (`DevDesc`) on AE coordinate differences per call:
// the arithmetic core of assemble_kernel / matvec_kernel (assemble.hip).  Kept in a header so that
// the host-only AddressSanitizer build (`build.sh --host-asan`, csrc/hosttest/) runs the SAME code on
// the CPU against the lowering under test.  Under hipcc this is device code; the host compiler sees
// plain C++ (that build is test infrastructure: nothing in the product calls the host instantiation).
#pragma once

#include <cmath>
#include <cstring>

#include "lpgp_desc.h"
#include "exp_table.h"

#if defined(__HIPCC__)
#define LPGP_HD __device__ __forceinline__
#else
#define LPGP_HD inline
#endif

namespace lpgp {

constexpr int AE = 8;           // entries per thread per pass (1 row x 8 cols)

LPGP_HD unsigned lpgp_hi32(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)__double2hiint(v);
#else
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  return (unsigned)(b >> 32);
#endif
}

// v with its sign bit XORed by `s` (s = 0 or 0x80000000)
LPGP_HD double lpgp_xor_sign(double v, unsigned s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hiloint2double((int)(((unsigned)__double2hiint(v)) ^ s), __double2loint(v));
#else
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  b ^= ((unsigned long long)s) << 32;
  std::memcpy(&v, &b, 8);
  return v;
#endif
}

// Where the exponential of a Matern dimension comes from.  A half-integer Matern factor decays like e^{-a |x - x'|}, and
//   e^{-a |x - x'|} = min( e^{-a (x - x0)} e^{+a (x' - x0)},  e^{+a (x - x0)} e^{-a (x' - x0)} )       (any origin x0)
// -- one of the two products is e^{-a |x - x'|} <= 1, the other its reciprocal -- so the per-ENTRY exponential of a tile of
// the block collapses into per-POINT exponentials (64 rows + 64 columns instead of 4096 entries) and two multiplies and a
// minimum per entry and dimension.  A provider with `enabled` hands out that minimum for (group, dimension, entry);
// `NoFactors` (the default) evaluates exp(-sum r_d) per entry as before.  Dimensions of squared-exponential kind keep their
// per-entry exponential (e^{-(u-u')^2/2} does not split without an exponential of the cross term), as do isotropic groups.
// Rounding: the argument a (x - x0) carries a relative error of one ulp, i.e. |a (x - x0)| eps absolute in the exponent, so the
// provider is only used while |a (x - x0)| stays below a small bound on the tile (assemble.hip: FACT_TMAX).
// The per-point factors E+ = e^{-a (x - x0)}, E- = e^{+a (x - x0)} with the argument carried in double-double: t = a (x - x0)
// = t_hi + t_lo exactly (TwoSum of the difference, FMA residual of the product), E+- = exp(-+t_hi) (1 -+ t_lo).  Without
// the low part the argument's rounding error, |t| eps, becomes a RELATIVE error of the entry -- also for near pairs x ~ x'
// far from the origin, where the direct evaluation exp(-a |x - x'|) is exact to an ulp; on Gram matrices of condition 1e9
// that moved the posterior by 3e-8 (tests/test_gpu_random.py, seed 107).  With it the entry carries the two exp roundings
// and one multiply, whatever the distance to the origin.
LPGP_HD void lpgp_exp_factors(double a, double x, double x0, double& ep, double& em, double& t_abs) {
  const double d_hi = x - x0;
  const double bb = d_hi - x;
  const double d_lo = (x - (d_hi - bb)) + (-x0 - bb);          // x - x0 = d_hi + d_lo exactly
  const double t_hi = a * d_hi;
  const double t_lo = fma(a, d_hi, -t_hi) + a * d_lo;
  const double e1 = exp(-t_hi), e2 = exp(t_hi);
  ep = fma(-t_lo, e1, e1);
  em = fma(t_lo, e2, e2);
  t_abs = fabs(t_hi);
}

// e^{-s} for s >= 0: the per-entry exponential of every assembly / matrix-free kernel.  The library exp costs 33 vector
// operations per entry inside these kernels (degree-11 Horner whose coefficients the compiler re-materialises per entry, range
// selects) out of ~71; this one costs 16 and one table read: s = r - k ln2/256 with |r| <= ln2/512, e^{-s} = 2^{k >> 8} T[k & 255]
// (1 + p(r)), T[j] = 2^{j/256} held as head + tail (exp_table.h), p a degree-4 polynomial of e^r - 1 (error 2.4e-18): the only
// rounding that matters is the final addition -- 0.51 ulp measured against quad precision over 2e7 arguments (the library's
// exp: 0.51 on the host, <= 1 documented on the device).  s is clamped at 800 (result 0); a NaN / infinite s reaches the entry
// through the polynomial factor that multiplies the exponential (its Horner chain starts from 0 * r), so it needs no branch
// here.  `tab`: 256 {head, tail} pairs -- LDS on the device (staged per workgroup), the constant itself on the host.
#if defined(__HIPCC__)
__device__ const double g_exp_table[2 * EXP_TAB_N] = {LPGP_EXP_TABLE_VALUES};
#else
static const double g_exp_table[2 * EXP_TAB_N] = {LPGP_EXP_TABLE_VALUES};
#endif

struct ExpTab {
  const double* t;
};

LPGP_HD double lpgp_exp_neg(double s, const ExpTab& tab) {
  const double t = -fmin(s, 800.0);
  const double kf = rint(t * EXP_N_OVER_LN2);
  double r = fma(kf, -EXP_LN2_N_HI, t);
  r = fma(kf, -EXP_LN2_N_LO, r);
  const int k = (int)kf;
  const double* tj = tab.t + 2 * (k & (EXP_TAB_N - 1));
  const double Th = tj[0], Tl = tj[1];
  double p = fma(r, EXP_C4, EXP_C3);
  p = fma(r, p, EXP_C2);
  p = fma(r, p, EXP_C1);
  p *= r;
  const double v = Th + fma(Th, p, Tl);
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ldexp(v, k >> EXP_TAB_BITS);
#else
  return std::ldexp(v, k >> EXP_TAB_BITS);
#endif
}

struct NoFactors {
  static constexpr bool enabled = false;
  LPGP_HD double pair(int, int, int) const { return 1.0; }
};

// Where the polynomial coefficients come from.  `MemCoef` reads the descriptor's table (scalar loads on the device).  Round 3
// tried a provider that keeps the whole table in ONE register pair spread over the lanes of the wave (a single coalesced load
// per kernel, two v_readlane per coefficient: no load-to-use latency inside the Horner loops): 2.81 against 2.89 TB/s on the
// 4096 x 16384 cross-covariance -- the scalar loads are not what bounds the kernel -- and it was removed again.
struct MemCoef {
  const double* base;
  LPGP_HD double operator()(int idx) const { return base[idx]; }
};

// One radial Matern group (LPGP_MATERN_RADIAL, DevGroup::iso == 2; layout: lpgp_desc.h, derivation: lower.cpp) added into res:
//   scale * e^{-s} * sum_m Theta_m(s) Pi_m(u),   u = a .* dx,  s = |u|,
// one sqrt, one reciprocal and one lpgp_exp_neg per entry.  Pi_m is a sparse list of monomials (the exponents are uniform: scalar
// loops of at most four multiplies), Theta_m a Horner chain in s plus, for m >= 3, a Horner chain in 1 / s that starts FROM Pi_m, so
// that every partial product stays bounded (a monomial of Pi_m has a higher degree than the most negative power it meets).  At
// s = 0 the reciprocal is replaced by 0 through a select: the negative powers then contribute h = 0 exactly (no 0 * inf), a
// non-constant monomial c * 0, and what remains is the diagonal value as lower.cpp stores it for desc_diag, operation for operation.
template <int D, int NE>
LPGP_HD void eval_radial_group(const DevDesc* __restrict__ desc, const DevGroup& G, const double (&dx)[D][NE], double (&res)[NE],
                               const ExpTab& tab) {
  double u[D][NE], s2[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) s2[e] = 0.0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const double a = G.a[j];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      u[j][e] = a * dx[j][e];
      s2[e] = fma(u[j][e], u[j][e], s2[e]);
    }
  }
  double sv[NE], inv[NE], tot[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    sv[e] = sqrt(s2[e]);
    inv[e] = sv[e] > 0.0 ? 1.0 / sv[e] : 0.0;
    tot[e] = 0.0;
  }
  const int p = G.deg[0];
  const int TL = rad_theta_len(p);
  const double* th = desc->coef + G.coef_off[0] + 1;
  const double* mono = desc->coef + G.coef_off[1];
#pragma unroll 1
  for (int m = 0; m < RAD_M; ++m, th += TL) {
    const int nm = G.parity[1 + m];
    if (nm == 0) continue;
    double pim[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) pim[e] = 0.0;
#pragma unroll 1
    for (int q = 0; q < nm; ++q, mono += 2) {
      const double c = mono[0];
      unsigned long long raw;
      __builtin_memcpy(&raw, mono + 1, 8);
      const unsigned bits = (unsigned)raw;
      double pr[NE];
#pragma unroll
      for (int e = 0; e < NE; ++e) pr[e] = 1.0;
#pragma unroll
      for (int j = 0; j < D; ++j)
        for (int k = (int)((bits >> (3 * j)) & 7u); k > 0; --k) {
#pragma unroll
          for (int e = 0; e < NE; ++e) pr[e] *= u[j][e];
        }
#pragma unroll
      for (int e = 0; e < NE; ++e) pim[e] = fma(c, pr[e], pim[e]);
    }
    double thv[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) thv[e] = 0.0;
    for (int k = p; k >= 0; --k) {
      const double c = th[k];
#pragma unroll
      for (int e = 0; e < NE; ++e) thv[e] = fma(thv[e], sv[e], c);
    }
    if (m >= 3) {
      const double n1 = th[p + 1], n2 = th[p + 2], n3 = th[p + 3];
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        double h = pim[e] * n3;
        h = fma(h, inv[e], pim[e] * n2);
        h = fma(h, inv[e], pim[e] * n1);
        h *= inv[e];
        tot[e] = fma(thv[e], pim[e], tot[e]) + h;
      }
    } else {
#pragma unroll
      for (int e = 0; e < NE; ++e) tot[e] = fma(thv[e], pim[e], tot[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < NE; ++e) res[e] = fma(G.scale * lpgp_exp_neg(sv[e], tab), tot[e], res[e]);
}

// (1 - r)^n for 0 <= r <= 1, n >= 0 uniform: a scalar loop of multiplies (Wendland groups; no exponential, no table read)
template <int NE>
LPGP_HD void lpgp_pow_1m(const double (&r)[NE], int n, double (&m)[NE]) {
  double t[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) t[e] = 1.0 - r[e];
  for (int k = n; k > 0; --k) {
#pragma unroll
    for (int e = 0; e < NE; ++e) m[e] *= t[e];
  }
}

// Which groups an instantiation may meet.  EV_RADIAL: radial Matern groups (iso == 2) too.  EV_COMPACT: everything -- Wendland
// dimensions and isotropic Wendland groups (expkind 3) beside all the other families, so that sums such as Wendland + Matern
// work.  The launch sites pick the variant on the host (desc_has_radial, desc_has_compact); EV_PLAIN never meets a radial or
// compact group and carries none of their code.
enum EvalVariant { EV_PLAIN = 0, EV_RADIAL = 1, EV_COMPACT = 2 };

template <int D, int NE, class Fac, class Coef, int VAR = EV_PLAIN>
LPGP_HD void eval_entries(const DevDesc* __restrict__ desc,
                                             const double (&dx)[D][NE], double (&res)[NE], const Fac& fac, const Coef& coef,
                                             const ExpTab& tab) {
  constexpr int AE = NE;          // (entries per call: the name the body uses)
#pragma unroll
  for (int e = 0; e < AE; ++e) res[e] = 0.0;
  for (int g = 0; g < desc->ngroups; ++g) {
    const DevGroup& G = desc->g[g];
    if constexpr (VAR != EV_PLAIN) {
      if (G.iso == 2) {
        eval_radial_group<D, NE>(desc, G, dx, res, tab);
        continue;
      }
    }
    if (G.iso) {
      // isotropic Matern: e^{-s} [Q0(s) + (w.u) Q1(s) + (u^T B u) Q2(s)],  u = a .* dx, s = |u|
      double s2[AE], lin[AE], quad[AE];
#pragma unroll
      for (int e = 0; e < AE; ++e) { s2[e] = 0.0; lin[e] = 0.0; quad[e] = 0.0; }
      double u[D][AE];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double a = G.a[j], wj = G.w[j];
#pragma unroll
        for (int e = 0; e < AE; ++e) {
          u[j][e] = a * dx[j][e];
          s2[e] = fma(u[j][e], u[j][e], s2[e]);
          lin[e] = fma(wj, u[j][e], lin[e]);
        }
      }
      if (G.has_quad) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double bu[AE];
#pragma unroll
          for (int e = 0; e < AE; ++e) bu[e] = 0.0;
#pragma unroll
          for (int j = 0; j < D; ++j) {
            const double bij = G.B[i * LPGP_MAXD + j];
#pragma unroll
            for (int e = 0; e < AE; ++e) bu[e] = fma(bij, u[j][e], bu[e]);
          }
#pragma unroll
          for (int e = 0; e < AE; ++e) quad[e] = fma(u[i][e], bu[e], quad[e]);
        }
      }
      const int q0 = G.coef_off[0], q1 = G.coef_off[1], q2 = G.coef_off[2];
      double sv[AE], v0[AE], v1[AE], v2[AE];
#pragma unroll
      for (int e = 0; e < AE; ++e) { sv[e] = sqrt(s2[e]); v0[e] = 0.0; v1[e] = 0.0; v2[e] = 0.0; }
      for (int k = G.deg[0]; k >= 0; --k) {
        const double c0 = coef(q0 + k), c1 = coef(q1 + k), c2 = coef(q2 + k);
#pragma unroll
        for (int e = 0; e < AE; ++e) {
          v0[e] = fma(v0[e], sv[e], c0);
          v1[e] = fma(v1[e], sv[e], c1);
          v2[e] = fma(v2[e], sv[e], c2);
        }
      }
      if constexpr (VAR == EV_COMPACT) {
        if (ek_kind(G.expkind[0]) == EK_COMPACT) {
          // isotropic Wendland: (1 - s)^pow inside the support (s^2 <= 1, so 1 - s >= 0), exactly 0.0 outside -- by a select,
          // not by a product with zero
          double cm[AE];
#pragma unroll
          for (int e = 0; e < AE; ++e) cm[e] = 1.0;
          lpgp_pow_1m<AE>(sv, ek_pow(G.expkind[0]), cm);
#pragma unroll
          for (int e = 0; e < AE; ++e) {
            const double v = fma(G.scale * cm[e], fma(quad[e], v2[e], fma(lin[e], v1[e], v0[e])), res[e]);
            res[e] = s2[e] <= 1.0 ? v : res[e];
          }
          continue;
        }
      }
#pragma unroll
      for (int e = 0; e < AE; ++e)
        res[e] = fma(G.scale * lpgp_exp_neg(sv[e], tab), fma(quad[e], v2[e], fma(lin[e], v1[e], v0[e])), res[e]);
      continue;
    }
    double r[D][AE];
    unsigned sg[D][AE];
    double expo[AE], ef[AE];
    bool per_entry_exp = !Fac::enabled && VAR != EV_COMPACT;       // some dimension of the group still needs exp(-expo) per entry
    bool inside[AE];                                               // EV_COMPACT: within the support of every Wendland dimension
#pragma unroll
    for (int e = 0; e < AE; ++e) { expo[e] = 0.0; ef[e] = 1.0; inside[e] = true; }
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const double a = G.a[j];
      const int kind = G.expkind[j];
#pragma unroll
      for (int e = 0; e < AE; ++e) {
        double v = a * dx[j][e];
        sg[j][e] = lpgp_hi32(v) & 0x80000000u;
        r[j][e] = fabs(v);
      }
      if constexpr (VAR == EV_COMPACT) {
        if (ek_kind(kind) == EK_COMPACT) {
          // a Wendland dimension: (1 - r)^pow inside the support (r <= 1), no exponential; outside, the select below
#pragma unroll
          for (int e = 0; e < AE; ++e) inside[e] = inside[e] && r[j][e] <= 1.0;
          lpgp_pow_1m<AE>(r[j], ek_pow(kind), ef);
          continue;
        }
      }
      if (Fac::enabled && kind == 1) {
#pragma unroll
        for (int e = 0; e < AE; ++e) ef[e] *= fac.pair(g, j, e);
      } else {
        per_entry_exp = true;
#pragma unroll
        for (int e = 0; e < AE; ++e) expo[e] += (kind == 1) ? r[j][e] : 0.5 * r[j][e] * r[j][e];
      }
    }
    double tot[AE];
#pragma unroll
    for (int e = 0; e < AE; ++e) tot[e] = 0.0;
    const int n1 = (D > 1) ? G.deg[D > 1 ? 1 : 0] + 1 : 1;
    const int n2 = (D > 2) ? G.deg[D > 2 ? 2 : 0] + 1 : 1;
    const int n3 = (D > 3) ? G.deg[D > 3 ? 3 : 0] + 1 : 1;
    for (int c = 0; c < G.ncls; ++c) {
      const int cf = G.coef_off[c];
      const int par = G.parity[c];
      double acc0[AE];
#pragma unroll
      for (int e = 0; e < AE; ++e) acc0[e] = 0.0;
      for (int i0 = G.deg[0]; i0 >= 0; --i0) {
        if constexpr (D == 1) {
          const double cv = coef(cf + i0);
#pragma unroll
          for (int e = 0; e < AE; ++e) acc0[e] = fma(acc0[e], r[0][e], cv);
        } else {
          double acc1[AE];
#pragma unroll
          for (int e = 0; e < AE; ++e) acc1[e] = 0.0;
          for (int i1 = n1 - 1; i1 >= 0; --i1) {
            if constexpr (D == 2) {
              const double cv = coef(cf + i0 * n1 + i1);
#pragma unroll
              for (int e = 0; e < AE; ++e) acc1[e] = fma(acc1[e], r[1][e], cv);
            } else {
              double acc2[AE];
#pragma unroll
              for (int e = 0; e < AE; ++e) acc2[e] = 0.0;
              for (int i2 = n2 - 1; i2 >= 0; --i2) {
                if constexpr (D == 3) {
                  const double cv = coef(cf + (i0 * n1 + i1) * n2 + i2);
#pragma unroll
                  for (int e = 0; e < AE; ++e) acc2[e] = fma(acc2[e], r[2][e], cv);
                } else {
                  double acc3[AE];
#pragma unroll
                  for (int e = 0; e < AE; ++e) acc3[e] = 0.0;
                  for (int i3 = n3 - 1; i3 >= 0; --i3) {
                    const double cv = coef(cf + ((i0 * n1 + i1) * n2 + i2) * n3 + i3);
#pragma unroll
                    for (int e = 0; e < AE; ++e) acc3[e] = fma(acc3[e], r[D - 1][e], cv);
                  }
#pragma unroll
                  for (int e = 0; e < AE; ++e) acc2[e] = fma(acc2[e], r[2][e], acc3[e]);
                }
              }
#pragma unroll
              for (int e = 0; e < AE; ++e) acc1[e] = fma(acc1[e], r[1][e], acc2[e]);
            }
          }
#pragma unroll
          for (int e = 0; e < AE; ++e) acc0[e] = fma(acc0[e], r[0][e], acc1[e]);
        }
      }
      // sign of the parity class: prod_{d in class} sign(x_d - x'_d)
#pragma unroll
      for (int e = 0; e < AE; ++e) {
        unsigned s = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) s ^= ((par >> j) & 1) ? sg[j][e] : 0u;
        double v = lpgp_xor_sign(acc0[e], s);
        tot[e] += v;
      }
    }
    if constexpr (VAR == EV_COMPACT) {
      // outside the support the group contributes nothing: a select, so that no (possibly negative or non-finite) power
      // of 1 - r > 1 ever meets the polynomial
      if (per_entry_exp) {
#pragma unroll
        for (int e = 0; e < AE; ++e) {
          const double v = fma(G.scale * (ef[e] * lpgp_exp_neg(expo[e], tab)), tot[e], res[e]);
          res[e] = inside[e] ? v : res[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < AE; ++e) {
          const double v = fma(G.scale * ef[e], tot[e], res[e]);
          res[e] = inside[e] ? v : res[e];
        }
      }
    } else if (per_entry_exp) {
#pragma unroll
      for (int e = 0; e < AE; ++e) res[e] = fma(G.scale * (ef[e] * lpgp_exp_neg(expo[e], tab)), tot[e], res[e]);
    } else {
#pragma unroll
      for (int e = 0; e < AE; ++e) res[e] = fma(G.scale * ef[e], tot[e], res[e]);
    }
  }
}

template <int D, int NE = AE, class Fac = NoFactors>
LPGP_HD void eval_entries(const DevDesc* __restrict__ desc, const double (&dx)[D][NE], double (&res)[NE], const ExpTab& tab,
                          const Fac& fac = Fac()) {
  eval_entries<D, NE, Fac, MemCoef>(desc, dx, res, fac, MemCoef{desc->coef}, tab);
}

// the same for a descriptor that may hold radial Matern groups
template <int D, int NE = AE>
LPGP_HD void eval_entries_radial(const DevDesc* __restrict__ desc, const double (&dx)[D][NE], double (&res)[NE], const ExpTab& tab) {
  eval_entries<D, NE, NoFactors, MemCoef, EV_RADIAL>(desc, dx, res, NoFactors(), MemCoef{desc->coef}, tab);
}

// the same for a descriptor of any kind, Wendland groups included
template <int D, int NE = AE>
LPGP_HD void eval_entries_compact(const DevDesc* __restrict__ desc, const double (&dx)[D][NE], double (&res)[NE], const ExpTab& tab) {
  eval_entries<D, NE, NoFactors, MemCoef, EV_COMPACT>(desc, dx, res, NoFactors(), MemCoef{desc->coef}, tab);
}

// by variant (the generic kernels of assemble.hip)
template <int VAR, int D, int NE>
LPGP_HD void eval_entries_var(const DevDesc* __restrict__ desc, const double (&dx)[D][NE], double (&res)[NE], const ExpTab& tab) {
  eval_entries<D, NE, NoFactors, MemCoef, VAR>(desc, dx, res, NoFactors(), MemCoef{desc->coef}, tab);
}

// Can NO entry between a row point in the box [rmin, rmax] and a column point in the box [cmin, cmax] lie inside the support of
// any group?  True only if every group is compact and out of reach: a product-form group through one Wendland dimension with
// a_j gap_j > 1, an isotropic Wendland group through sum_j (a_j gap_j)^2 > 1, gap_j the distance between the two intervals.
// The decision runs the operations of the entries themselves -- a difference of two coordinates, the product with a_j, the
// same fma chain, the same comparison -- on arguments that bound every entry's from below; rounding is monotone, so the decision
// implies the per-entry selects above and a block is bit-identical with and without the shortcut.
template <int D>
LPGP_HD bool lpgp_out_of_reach(const DevDesc* __restrict__ desc, const double (&rmin)[D], const double (&rmax)[D], const double (&cmin)[D],
                               const double (&cmax)[D]) {
  double gap[D];
#pragma unroll
  for (int j = 0; j < D; ++j) gap[j] = fmax(fmax(rmin[j] - cmax[j], cmin[j] - rmax[j]), 0.0);
  bool out = true;
  for (int g = 0; g < desc->ngroups; ++g) {
    const DevGroup& G = desc->g[g];
    bool far = false;
    if (G.iso) {
      if (G.iso == 1 && ek_kind(G.expkind[0]) == EK_COMPACT) {
        double s2 = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const double u = G.a[j] * gap[j];
          s2 = fma(u, u, s2);
        }
        far = !(s2 <= 1.0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < D; ++j)
        if (ek_kind(G.expkind[j]) == EK_COMPACT && !(fabs(G.a[j] * gap[j]) <= 1.0)) far = true;
    }
    out = out && far;
  }
  return out;
}

}  // namespace lpgp
