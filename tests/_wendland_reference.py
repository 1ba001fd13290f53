"""Exact and fp64 references of the Wendland families (`LPGP_WENDLAND`, `LPGP_WENDLAND_ISO`), independent of csrc/lower.cpp.

phi_{d,k} is built from the definition (Wendland 2004, Def. 9.11): l = floor(d/2) + k + 1, phi = I^k (1 - r)_+^l with
(I f)(r) = int_r^1 t f(t) dt, normalised to phi(0) = 1, in `fractions.Fraction`.  Blocks (L0 k L1'^*)(X0, X1) are evaluated
 * exactly (`exact_block`): at the exact rational values of the fp64 inputs, from the POWER-BASIS coefficients of phi and
   its derivatives (no factoring involved).  What is irrational -- the radius of the isotropic kernel, the exponential and the
   sqrt(5) of a Matern-5/2 factor beside a Wendland factor -- is carried in rationals accurate to 2^-256;
 * with an envelope E: the sums of the evaluation form the library is specified to use -- per dimension the common power
   (1 - r)^{m - nmax} times, per term, the polynomial (1 - r)^{nmax - n} q_n(r) expanded in r; for the isotropic kernel
   (1 - s)^{m - o} [Q0 + (w.u) Q1 + (u^T B u) Q2] -- with the absolute value of every coefficient, monomial and term.  The
   power (1 - r)^e is computed from a ROUNDED r (x - x' and 1 / lengthscale are rounded): its absolute error is
   e (1 - r)^{e-1} r eps, not a relative one, so the envelope carries the power e - 1 (for e >= 1).  E is what an error of
   the evaluation is measured in: |got - exact| <= K eps E;
 * in fp64 NumPy in the factored form (`helper_block`).
Kernel specs: ("prod", [(fam, k_or_p, lengthscale), ...]) with fam "w" (Wendland phi_{1,k}) or "m" (Matern nu = p + 1/2), or
("iso", k, [lengthscales]).  A kernel is a list of (scale, spec): a sum.  Operators: {multi-index: coefficient} maps.
"""
from fractions import Fraction
from math import comb, isqrt

import numpy as np

EPS = 2.0**-53
FX = 256                      # bits of the rationals that stand for irrational numbers

# HELPER_BOUND, from the operations of `helper_block` (each counted as one relative rounding eps, first order):
#  r: 1 / lengthscale, x - x', their product: 3 roundings.  They reach an entry through (1 - r)^e, as 3 e r (1 - r)^{e-1} eps <=
#  3 e eps E (the envelope carries the power e - 1), e <= 9; and through the polynomials (degree <= 9), as <= 3 * 9 eps E: 54.
#  (1 - r)^e: e - 1 <= 8 multiplies; Horner: 2 * 9 roundings and the rounded coefficients, 10; sign, scale, prefactor a^n: 4.
#  About 95 per dimension; the dimensions of a product multiply (errors add: x 2 in the 2-D blocks tested), and the terms add
#  within E.  An isotropic entry adds sqrt and the two fma chains (<= 12) to one such count.  2 x 95 + margin:
HELPER_BOUND = 256.0
# Worst |helper - exact| / (eps E) over every block of tests/test_wendland_host.py::test_numpy_helper_vs_exact (it prints the
# figure).  The device is allowed 4x that (another order of summation, fma contraction, the table exponential of a Matern
# factor): K_DEVICE, used by csrc/hosttest/wendland_check.cpp and tests/test_gpu_wendland.py.
HELPER_WORST_MEASURED = 10.90
K_DEVICE = 4 * HELPER_WORST_MEASURED        # 43.6


# ---------------------------------------------------------------------------------------------------------------------
# polynomials (lists of Fractions, ascending powers)
# ---------------------------------------------------------------------------------------------------------------------
def _trim(p):
    p = list(p)
    while len(p) > 1 and p[-1] == 0:
        p.pop()
    return p


def _mul(p, q):
    out = [Fraction(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def _add(p, q, sq=1):
    n = max(len(p), len(q))
    return [(p[i] if i < len(p) else 0) + sq * (q[i] if i < len(q) else 0) for i in range(n)]


def _der(p, n=1):
    p = list(p)
    for _ in range(n):
        p = [i * c for i, c in enumerate(p)][1:] or [Fraction(0)]
    return p


def _div_1mr(p, e):
    """p / (1 - r)^e, which must be exact."""
    p = _trim(p)
    for _ in range(e):
        q = [p[0]]
        for c in p[1:]:
            q.append(c + q[-1])
        assert q[-1] == 0, "not divisible by (1 - r)"
        p = q[:-1] or [Fraction(0)]
    return p


def _shift_down(p, n):
    """p / r^n, which must be exact."""
    assert all(c == 0 for c in p[:n]), "not divisible by a power of r"
    return list(p[n:]) or [Fraction(0)]


ONE_MINUS_R = [Fraction(1), Fraction(-1)]


def _pow_1mr(e):
    out = [Fraction(1)]
    for _ in range(e):
        out = _mul(out, ONE_MINUS_R)
    return out


def _peval(p, x):
    acc = 0
    for c in reversed(p):
        acc = acc * x + c
    return acc


def phi(d, k):
    """Power-basis coefficients of phi_{d,k} on [0, 1]."""
    l = d // 2 + k + 1
    f = [Fraction(comb(l, i) * (-1) ** i) for i in range(l + 1)]
    for _ in range(k):
        g = [Fraction(0)] * (len(f) + 2)
        for j, c in enumerate(f):
            g[0] += c / (j + 2)
            g[j + 2] -= c / (j + 2)
        f = g
    return [c / f[0] for c in f]


def m_of(d, k):
    return d // 2 + 2 * k + 1


def factored(d, k, n=0):
    """(e, q): phi_{d,k}^(n)(r) = (1 - r)^e q(r), e = m - n."""
    e = m_of(d, k) - n
    return e, _div_1mr(_der(phi(d, k), n), e)


def matern_polys(p, nmax):
    """P_0 .. P_nmax: d^n/dr^n [P_0(r) e^{-r}] = P_n(r) e^{-r}, kappa = P_0 e^{-r} the Matern function of nu = p + 1/2 in r."""
    from math import factorial as f
    den = Fraction(f(2 * p), f(p))
    out = [[Fraction(f(2 * p - i) * 2**i, f(p - i) * f(i)) / den for i in range(p + 1)]]
    for _ in range(nmax):
        out.append(_add(_der(out[-1]), out[-1], -1))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# irrational numbers as rationals good to 2^-FX
# ---------------------------------------------------------------------------------------------------------------------
def sqrt_frac(q):
    q = Fraction(q)
    return Fraction(isqrt((q.numerator << (2 * FX + 64)) // q.denominator), 1 << (FX + 32))


def exp_neg_frac(r):
    """e^{-r}, r >= 0 rational."""
    r = Fraction(r)
    y = r / (1 << 12)
    term, acc = Fraction(1), Fraction(1)
    for i in range(1, 40):
        term = term * (-y) / i
        term = Fraction((term.numerator << (FX + 64)) // term.denominator, 1 << (FX + 64))
        acc += term
    for _ in range(12):
        acc = acc * acc
        acc = Fraction((acc.numerator << (FX + 64)) // acc.denominator, 1 << (FX + 64))
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# exact blocks and envelopes
# ---------------------------------------------------------------------------------------------------------------------
def _terms(L0, L1):
    out = {}
    for a0, c0 in L0.items():
        for a1, c1 in L1.items():
            key = (tuple(a0), tuple(a1))
            out[key] = out.get(key, 0.0) + c0 * c1
    return [(Fraction(c), a0, a1) for (a0, a1), c in out.items() if c != 0.0]


class _ProdDim:
    """One dimension of a product-form group: exact value and envelope of the order-n factor at a scaled distance."""

    def __init__(self, fam, kp, ls, orders):
        self.fam, self.kp = fam, kp
        self.nmax = max(orders)
        if fam == "w":
            self.a = 1 / Fraction(ls)
            self.m = m_of(1, kp)
            assert self.nmax <= 2 * kp
            self.power = {n: _der(phi(1, kp), n) for n in set(orders)}
            # what the group keeps per order: (1 - r)^{nmax - n} q_n(r), expanded; the common power is m - nmax
            self.stored = {n: _mul(_pow_1mr(self.nmax - n), factored(1, kp, n)[1]) for n in set(orders)}
        else:
            self.a = sqrt_frac(2 * kp + 1) / Fraction(ls)
            self.power = dict(enumerate(matern_polys(kp, self.nmax)))
            self.stored = self.power
        self._cache = {}

    def at(self, delta, n):
        """(value, envelope, outside) of a^n sign^n phi^(n)(a |delta|) (the factor (-1)^{n1} is the caller's)."""
        key = (delta, n)
        if key in self._cache:
            return self._cache[key]
        r = abs(delta) * self.a
        sgn = -1 if (delta < 0 and n % 2) else 1
        an = self.a**n
        if self.fam == "w":
            if r > 1:
                res = (Fraction(0), Fraction(0), True)
            else:
                e = self.m - self.nmax
                env = (1 - r) ** max(e - 1, 0) * _peval([abs(c) for c in self.stored[n]], r)
                res = (sgn * an * _peval(self.power[n], r), an * env, False)
        else:
            ex = self._cache.get(("exp", r))
            if ex is None:
                ex = self._cache[("exp", r)] = exp_neg_frac(r)
            res = (sgn * an * ex * _peval(self.power[n], r), an * ex * _peval([abs(c) for c in self.stored[n]], r), False)
        self._cache[key] = res
        return res


def _exact_prod(factors, terms, X0, X1, G, E, OUT):
    d = len(factors)
    dims = [_ProdDim(f[0], f[1], f[2], [a0[j] + a1[j] for _, a0, a1 in terms]) for j, f in enumerate(factors)]
    F0 = [[Fraction(float(v)) for v in row] for row in X0]
    F1 = [[Fraction(float(v)) for v in row] for row in X1]
    for i, x in enumerate(F0):
        for jj, y in enumerate(F1):
            delta = [x[q] - y[q] for q in range(d)]
            val = env = Fraction(0)
            outside = True
            for c, a0, a1 in terms:
                v, e = c * (-1) ** (sum(a1) % 2), abs(c)
                for q in range(d):
                    fv, fe, fo = dims[q].at(delta[q], a0[q] + a1[q])
                    v, e = v * fv, e * fe
                    if fo:
                        break
                else:
                    outside = False
                    val += v
                    env += e
            G[i][jj] += val
            E[i][jj] += env
            OUT[i][jj] = OUT[i][jj] and outside


def _exact_iso(k, ls, terms, X0, X1, G, E, OUT):
    d = len(ls)
    a = [1 / Fraction(float(l)) for l in ls]
    ph = phi(d, k)
    orders = [sum(a0) + sum(a1) for _, a0, a1 in terms]
    o = max(orders)
    assert all(sum(a0) <= 1 and sum(a1) <= 1 for _, a0, a1 in terms) and (o == 0 or k >= 1) and (o < 2 or k >= 2)
    m = m_of(d, k)
    # exact: phi, F1 = phi'/s, F2 = (phi'' - phi'/s)/s^2 in the power basis
    F1 = _shift_down(_der(ph), 1) if o >= 1 else [Fraction(0)]
    F2 = _shift_down(_add(_der(ph, 2), F1, -1), 2) if o >= 2 else [Fraction(0)]
    # envelope: the polynomials of the specified form, common power (1 - s)^{m - o}
    q0 = [abs(c) for c in _mul(_pow_1mr(o), factored(d, k, 0)[1])]
    q1s = q2s = [Fraction(0)]
    if o >= 1:
        q1s = _shift_down(_mul(_pow_1mr(o - 1), factored(d, k, 1)[1]), 1)
    if o >= 2:
        q2s = [abs(c) for c in _shift_down(_add(factored(d, k, 2)[1], _shift_down(_mul(ONE_MINUS_R, factored(d, k, 1)[1]), 1), -1), 2)]
    q1s = [abs(c) for c in q1s]
    F0_ = [[Fraction(float(v)) for v in row] for row in X0]
    F1_ = [[Fraction(float(v)) for v in row] for row in X1]
    for i, x in enumerate(F0_):
        for jj, y in enumerate(F1_):
            u = [a[q] * (x[q] - y[q]) for q in range(d)]
            s2 = sum(v * v for v in u)
            if s2 > 1:
                continue
            OUT[i][jj] = False
            s = sqrt_frac(s2)
            v0, v1, v2 = _peval(ph, s), _peval(F1, s), _peval(F2, s)
            e0, e1, e2 = _peval(q0, s), _peval(q1s, s), _peval(q2s, s)
            val = env = Fraction(0)
            for c, a0, a1 in terms:
                o0, o1 = sum(a0), sum(a1)
                if not o0 and not o1:
                    val += c * v0
                    env += abs(c) * e0
                elif o0 and not o1:
                    q = a0.index(1)
                    val += c * a[q] * u[q] * v1
                    env += abs(c * a[q] * u[q]) * e1
                elif o1 and not o0:
                    q = a1.index(1)
                    val -= c * a[q] * u[q] * v1
                    env += abs(c * a[q] * u[q]) * e1
                else:
                    q0_, q1_ = a0.index(1), a1.index(1)
                    val -= c * a[q0_] * a[q1_] * u[q0_] * u[q1_] * v2
                    env += abs(c * a[q0_] * a[q1_] * u[q0_] * u[q1_]) * e2
                    if q0_ == q1_:
                        val -= c * a[q0_] ** 2 * v1
                        env += abs(c) * a[q0_] ** 2 * e1
            G[i][jj] += val
            E[i][jj] += (1 - s) ** max(m - o - 1, 0) * env


def exact_block(kernel, L0, L1, X0, X1):
    """(G, E, outside): float64 arrays of the exact block, its envelope, and the mask of entries outside every summand's support."""
    X0, X1 = np.asarray(X0, dtype=np.double), np.asarray(X1, dtype=np.double)
    if X0.ndim == 1:
        X0, X1 = X0[:, None], X1[:, None]
    n0, n1 = X0.shape[0], X1.shape[0]
    G = [[Fraction(0)] * n1 for _ in range(n0)]
    E = [[Fraction(0)] * n1 for _ in range(n0)]
    OUT = [[True] * n1 for _ in range(n0)]
    terms = _terms(L0, L1)
    for scale, spec in kernel:
        Gs = [[Fraction(0)] * n1 for _ in range(n0)]
        Es = [[Fraction(0)] * n1 for _ in range(n0)]
        if spec[0] == "prod":
            _exact_prod(spec[1], terms, X0, X1, Gs, Es, OUT)
        else:
            _exact_iso(spec[1], spec[2], terms, X0, X1, Gs, Es, OUT)
        sc = Fraction(float(scale))
        for i in range(n0):
            for j in range(n1):
                G[i][j] += sc * Gs[i][j]
                E[i][j] += abs(sc) * Es[i][j]
    tofl = lambda M: np.array([[float(v) for v in row] for row in M], dtype=np.double)  # noqa: E731
    return tofl(G), tofl(E), np.array(OUT, dtype=bool)


def identity(d):
    return {(0,) * d: 1.0}


# ---------------------------------------------------------------------------------------------------------------------
# fp64 NumPy helper in the factored form
# ---------------------------------------------------------------------------------------------------------------------
def _horner(p, x):
    acc = np.zeros_like(x)
    for c in reversed(p):
        acc = acc * x + float(c)
    return acc


def helper_block(kernel, L0, L1, X0, X1):
    X0, X1 = np.asarray(X0, dtype=np.double), np.asarray(X1, dtype=np.double)
    if X0.ndim == 1:
        X0, X1 = X0[:, None], X1[:, None]
    dx = X0[:, None, :] - X1[None, :, :]
    terms = [(float(c), a0, a1) for c, a0, a1 in _terms(L0, L1)]
    out = np.zeros(dx.shape[:2])
    for scale, spec in kernel:
        if spec[0] == "prod":
            factors = spec[1]
            grp = np.zeros(dx.shape[:2])
            for c, a0, a1 in terms:
                v = np.full(dx.shape[:2], c * (-1.0) ** (sum(a1) % 2))
                for q, (fam, kp, ls) in enumerate(factors):
                    n = a0[q] + a1[q]
                    if fam == "w":
                        a = 1.0 / ls
                        u = a * dx[:, :, q]
                        r = np.abs(u)
                        e, poly = factored(1, kp, n)
                        f = np.where(r <= 1.0, (1.0 - np.minimum(r, 1.0)) ** e * _horner(poly, r), 0.0)
                    else:
                        a = np.sqrt(2.0 * (kp + 0.5)) / ls
                        u = a * dx[:, :, q]
                        r = np.abs(u)
                        f = np.exp(-r) * _horner(matern_polys(kp, n)[n], r)
                    v = v * (a**n * np.where((u < 0) & (n % 2 == 1), -1.0, 1.0) * f)
                grp += v
            out += scale * grp
        else:
            k, ls = spec[1], np.asarray(spec[2], dtype=np.double)
            d = len(ls)
            a = 1.0 / ls
            u = a[None, None, :] * dx
            s2 = np.sum(u * u, axis=-1)
            s = np.sqrt(s2)
            m = m_of(d, k)
            t = 1.0 - np.minimum(s, 1.0)
            _, q0 = factored(d, k, 0)
            ph = t**m * _horner(q0, s)
            o = max(sum(a0) + sum(a1) for _, a0, a1 in terms)
            f1 = f2 = None
            if o >= 1:
                q1s = _shift_down(factored(d, k, 1)[1], 1)
                f1 = t ** (m - 1) * _horner(q1s, s)
            if o >= 2:
                q2s = _shift_down(_add(factored(d, k, 2)[1], _shift_down(_mul(ONE_MINUS_R, factored(d, k, 1)[1]), 1), -1), 2)
                f2 = t ** (m - 2) * _horner(q2s, s)
            grp = np.zeros(dx.shape[:2])
            for c, a0, a1 in terms:
                o0, o1 = sum(a0), sum(a1)
                if not o0 and not o1:
                    grp += c * ph
                elif o0 and not o1:
                    q = a0.index(1)
                    grp += c * a[q] * u[:, :, q] * f1
                elif o1 and not o0:
                    q = a1.index(1)
                    grp -= c * a[q] * u[:, :, q] * f1
                else:
                    i0, i1 = a0.index(1), a1.index(1)
                    grp -= c * a[i0] * a[i1] * u[:, :, i0] * u[:, :, i1] * f2
                    if i0 == i1:
                        grp -= c * a[i0] ** 2 * f1
            out += scale * np.where(s2 <= 1.0, grp, 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases shared by tests/test_wendland_host.py (small blocks, on the CPU) and tests/test_gpu_wendland.py (150 x 70)
# ---------------------------------------------------------------------------------------------------------------------
def base_groups(kernel):
    """The kernel as the `base_groups` of `covfuncs.lower_groups`: [(scale, [(family, p, lengthscale), ...])]."""
    out = []
    for scale, spec in kernel:
        if spec[0] == "prod":
            out.append((float(scale), [(5 if f == "w" else 1, int(kp), float(ls)) for f, kp, ls in spec[1]]))
        else:
            out.append((float(scale), [(6, int(spec[1]), float(l)) for l in spec[2]]))
    return out


def _e(d, i, n=1):
    return tuple(n if j == i else 0 for j in range(d))


def derivative_cases():
    """[(name, kernel, L0, L1)]: the derivative blocks both test files hold to the exact values."""
    cases = []
    # D = 1: every (n0, n1) with n0 + n1 <= 2 k
    for k in (1, 2, 3):
        kern = [(1.0, ("prod", [("w", k, 0.7)]))]
        for n0 in range(2 * k + 1):
            for n1 in range(2 * k + 1 - n0):
                cases.append((f"1d_k{k}_d{n0}_d{n1}", kern, {(n0,): 1.0}, {(n1,): 1.0}))
    # D = 2 tensor products
    ident, mlap = identity(2), {(2, 0): -1.0, (0, 2): -1.0}
    mixed0, mixed1 = {(1, 0): 0.5, (0, 2): -1.0, (0, 0): 2.0}, {(0, 1): 1.5, (2, 0): 0.25}
    ww = [(1.3, ("prod", [("w", 2, 0.7), ("w", 3, 0.9)]))]
    wm = [(0.8, ("prod", [("w", 2, 0.8), ("m", 2, 0.6)]))]
    for tag, kern in (("ww", ww), ("wm", wm)):
        cases.append((f"2d_{tag}_lap_id", kern, mlap, ident))
        cases.append((f"2d_{tag}_lap_lap", kern, mlap, mlap))
        cases.append((f"2d_{tag}_mixed", kern, mixed0, mixed1))
    # isotropic
    for d in (2, 3):
        ls = [0.9, 0.7, 1.1][:d]
        v = {_e(d, i): c for i, c in enumerate([1.0, -0.5, 0.75][:d])}
        w = {_e(d, i): c for i, c in enumerate([0.25, 2.0, -1.0][:d])}
        cases.append((f"iso_d{d}_k1_id_dir", [(1.0, ("iso", 1, ls))], identity(d), w))
        for k in (2, 3):
            v1 = dict(v)
            v1[(0,) * d] = 0.5
            cases.append((f"iso_d{d}_k{k}_dir_dir", [(1.1, ("iso", k, ls))], v1, w))
    # a sum Wendland + Matern
    cases.append(("sum_w_m", [(1.0, ("prod", [("w", 2, 0.6), ("w", 2, 0.8)])), (0.5, ("prod", [("m", 2, 0.9), ("m", 1, 1.2)]))],
                  {(1, 0): 1.0, (0, 0): 0.5}, {(0, 1): 1.0, (0, 0): 1.0}))
    return cases


def dyadic_points(rng, n, d, bits=6):
    """Points of [-1, 1]^d on the grid 2^-bits: differences are exact and repeat, so the exact blocks stay cheap."""
    return rng.integers(-(1 << bits), (1 << bits) + 1, (n, d)).astype(np.double) / (1 << bits)


# ---------------------------------------------------------------------------------------------------------------------
# the posterior problem (tests/test_wendland_host.py on the CPU, tests/test_gpu_wendland.py on the device)
# ---------------------------------------------------------------------------------------------------------------------
POST_KERNEL = [(1.0, ("prod", [("w", 2, 0.7), ("w", 2, 0.7)]))]
POST_NUGGET = 1e-8


def posterior_problem():
    g = np.linspace(-0.9, 0.9, 10)
    Xc = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    t = np.linspace(-1.0, 1.0, 13)[:-1]
    Xb = np.concatenate([np.column_stack([-np.ones(12), t]), np.column_stack([t + 2.0 / 12, -np.ones(12)]),
                         np.column_stack([np.ones(12), t + 2.0 / 12]), np.column_stack([t, np.ones(12)])])
    p = np.linspace(-0.95, 0.95, 8)
    Xt = np.stack(np.meshgrid(p, p, indexing="ij"), axis=-1).reshape(-1, 2)
    return Xc, np.full(100, 2.0), Xb, np.zeros(48), Xt


def posterior_matrices():
    """G (148 x 148, the nugget on the boundary block), K_Xx (148 x 64), k_xx (64), y (148) by the fp64 helper."""
    Xc, yc, Xb, yb, Xt = posterior_problem()
    ident, mlap = identity(2), {(2, 0): -1.0, (0, 2): -1.0}
    Gcc = helper_block(POST_KERNEL, mlap, mlap, Xc, Xc)
    Gbc = helper_block(POST_KERNEL, ident, mlap, Xb, Xc)
    Gbb = helper_block(POST_KERNEL, ident, ident, Xb, Xb) + POST_NUGGET * np.eye(48)
    G = np.block([[Gcc, Gbc.T], [Gbc, Gbb]])
    Kx = np.concatenate([helper_block(POST_KERNEL, mlap, ident, Xc, Xt), helper_block(POST_KERNEL, ident, ident, Xb, Xt)])
    return G, Kx, np.ones(64), np.concatenate([yc, yb])


def posterior_lapack():
    """Posterior mean, variance, log marginal likelihood and leave-one-out mean / variance by fp64 LAPACK (zero prior mean)."""
    G, Kx, kxx, y = posterior_matrices()
    L = np.linalg.cholesky(G)
    w = np.linalg.solve(G, y)
    V = np.linalg.solve(L, Kx)
    mean, var = Kx.T @ w, kxx - np.sum(V * V, axis=0)
    lml = -0.5 * y @ w - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi)
    Ginv_diag = np.sum(np.linalg.solve(L, np.eye(len(y))) ** 2, axis=0)
    return {"mean": mean, "var": var, "lml": float(lml), "loo_mean": y - w / Ginv_diag, "loo_var": 1.0 / Ginv_diag, "cond": float(np.linalg.cond(G))}


def posterior_refined():
    """The same from solves refined in long double (residuals and updates in np.longdouble, corrections by the fp64 factor)."""
    G, Kx, kxx, y = posterior_matrices()
    Gl = G.astype(np.longdouble)

    def solve(B):
        B = np.asarray(B, dtype=np.longdouble)
        X = np.zeros_like(B)
        for _ in range(8):
            R = B - Gl @ X
            X = X + np.linalg.solve(G, R.astype(np.double)).astype(np.longdouble)
        return X

    w = solve(y)
    S = solve(Kx)
    Kl = Kx.astype(np.longdouble)
    mean, var = Kl.T @ w, kxx - np.sum(Kl * S, axis=0)
    Ginv_diag = np.diag(solve(np.eye(len(y))))
    return {"mean": mean.astype(np.double), "var": var.astype(np.double), "loo_mean": (y - w / Ginv_diag).astype(np.double),
            "loo_var": (1.0 / Ginv_diag).astype(np.double)}
