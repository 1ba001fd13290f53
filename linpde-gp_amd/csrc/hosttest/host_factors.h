// The host twin of the per-point exponential factors (eval_entries.h: `Fac`; on the device the factors sit in LDS, assemble.hip:
// LdsFactors): per-point exponentials e^{-+ a (x - x0)} of every Matern dimension relative to an origin x0, the per-entry
// exponential as the minimum of the two products -- the SAME eval_entries code path.  Shared by the host test library
// (host_check.cpp) and the stand-alone entry check (entries_check.cpp).
#pragma once

#include "../eval_entries.h"

namespace lpgp {

template <int D, int NE = AE>
struct HostFactors {
  static constexpr bool enabled = true;
  const DevDesc* desc;
  double xr[D], xc[D][NE], x0[D];
  double pair(int g, int j, int e) const {
    const double a = desc->g[g].a[j];
    double rp, rm, cp, cm, t;
    lpgp_exp_factors(a, xr[j], x0[j], rp, rm, t);
    lpgp_exp_factors(a, xc[j][e], x0[j], cp, cm, t);
    const double p1 = rp * cm, p2 = rm * cp;
    return p1 < p2 ? p1 : p2;
  }
};

}  // namespace lpgp
