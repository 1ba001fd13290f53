"""Straightforward NumPy fp64 evaluation of second-order operators on the isotropic Matern kernel (the radial closed form).

Independent of csrc/lower.cpp: rational Theta_m from `fractions`, the expansion of d_u^alpha psi term by term, no tables shared
with the library.  With u = a .* (x - x'), s = |u|, t = s^2 / 2, psi(t) = kappa(s):
    d_u^alpha psi = sum_{j <= alpha/2} psi^(|alpha|-|j|)(t) prod_d alpha_d! / (j_d! (alpha_d - 2 j_d)! 2^j_d) u_d^(alpha_d - 2 j_d)
    psi^(m) = e^{-s} Theta_m(s),  Theta_0 = P_p,  Theta_{m+1} = (Theta_m' - Theta_m) / s        (Laurent polynomials in s)
    d/dx_i = a_i d/du_i,  d/dx'_i = -a_i d/du_i.
`block(...)` returns (L0 k L1'^*)(X0, X1) for operators given as {multi-index: coefficient} maps.
"""
import itertools
from fractions import Fraction
from math import factorial

import numpy as np

# Worst |helper - golden| / (eps * E) of `block` over every entry of tests/golden/iso_radial.npz (E: the stored envelope, eps = 2^-53),
# measured on the CPU by tests/test_iso_radial_host.py::test_numpy_helper_vs_golden (it prints the figure); MEASUREMENTS.md.
# The worst entries are the pairs at s ~ 50: the rounding of s (and of x - x' before it) is an error of s * eps in the exponent.
# The device is allowed 4x that (table exponential, another order of summation): K_DEVICE.  The helper itself is held to 2x,
# the room another libm's exp and pow may take.
HELPER_WORST_MEASURED = 132.94
HELPER_BOUND = 2 * HELPER_WORST_MEASURED
K_DEVICE = 4 * HELPER_WORST_MEASURED        # 531.76


def theta(p):
    """[Theta_0 .. Theta_4], each {power of s: Fraction}."""
    den = Fraction(factorial(2 * p), factorial(p))
    th = [{k: Fraction(factorial(2 * p - k) * 2**k, factorial(p - k) * factorial(k)) / den for k in range(p + 1)}]
    for _ in range(4):
        cur, nxt = th[-1], {}
        for k, c in cur.items():
            nxt[k - 2] = nxt.get(k - 2, 0) + k * c       # derivative, divided by s
            nxt[k - 1] = nxt.get(k - 1, 0) - c
        th.append({k: c for k, c in nxt.items() if c != 0})
    return th


def block(p, lengthscales, L0, L1, X0, X1, scale=1.0):
    X0, X1 = np.atleast_2d(np.asarray(X0, dtype=np.double)), np.atleast_2d(np.asarray(X1, dtype=np.double))
    d = X0.shape[1]
    a = np.sqrt(2.0 * (p + 0.5)) / np.broadcast_to(np.asarray(lengthscales, dtype=np.double), (d,))
    u = a[None, None, :] * (X0[:, None, :] - X1[None, :, :])
    s = np.sqrt(np.sum(u * u, axis=-1))
    zero = s == 0
    s_safe = np.where(zero, 1.0, s)
    th = theta(p)
    out = np.zeros(s.shape)
    for al0, c0 in L0.items():
        for al1, c1 in L1.items():
            al = tuple(x + y for x, y in zip(al0, al1))
            pref = c0 * c1 * (-1.0) ** sum(al1) * float(np.prod(a ** np.array(al)))
            if pref == 0.0:
                continue
            for jj in itertools.product(*[range(k // 2 + 1) for k in al]):
                w = pref
                mono = np.ones(s.shape)
                for k, j, ud in zip(al, jj, np.moveaxis(u, -1, 0)):
                    w *= factorial(k) / (factorial(j) * factorial(k - 2 * j) * 2**j)
                    mono = mono * ud ** (k - 2 * j)
                m = sum(al) - sum(jj)
                for pw, co in th[m].items():
                    if pw >= 0:
                        out += w * float(co) * mono * s**pw
                    else:
                        if sum(al) - 2 * sum(jj) <= -pw:
                            raise ValueError("not differentiable enough: a singular term without a vanishing monomial")
                        out += np.where(zero, 0.0, w * float(co) * mono / s_safe ** (-pw))
    return scale * np.exp(-s) * out
