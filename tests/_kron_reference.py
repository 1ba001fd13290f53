"""High-precision reference of one tensor-grid block of the Gram matrix, its componentwise error envelope, and the case list of
the entry-exact suites (test_kron_reference.py on the CPU, test_gpu_kron_exact.py on the device).  A plain module, not a conftest.

Independent of the device code, of `csrc/lower.cpp` and of `oracle/`: a 1-D factor d^{n0}/dx^{n0} d^{n1}/dx'^{n1} k_d(x, x') is the
textbook closed form of the half-integer Matern / squared-exponential kernel differentiated symbolically by SymPy, reduced to
polynomial(r) * exponential, and evaluated with mpmath at `DPS` digits on the exact binary values of the coordinates.  Its
ENVELOPE is the same expression with every polynomial coefficient replaced by its absolute value (and |r| for r): a rounding
error of a few ulp in the exponential, in any Horner step or in the argument moves the value by a few eps of the envelope, also
where the derivative itself crosses zero, which is what makes an entry-by-entry bound possible.

The block  G[(i_0..i_{D-1}), (j_0..j_{D-1})] = sum_t c_t prod_d M_{t,d}[i_d, j_d]  and its envelope  E = sum_t |c_t| prod_d E_{t,d}
are formed in `np.longdouble` by `np.kron` on the C-order mesh (last dimension fastest)."""
import functools
import itertools
import math

import mpmath
import numpy as np
import sympy as sp

DPS = 34
LD = np.longdouble
EPS = 2.0 ** -53          # unit roundoff of float64


# ---- 1-D factors ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _matern_polys(p, n0, n1):
    """d^{n0}_x d^{n1}_y kappa_p(a |x - y|) = q(r) e^{-a r}, r = |x - y|: the coefficients of q (lowest first, expressions in `a`) on
    the branch x > y and on the branch x < y, as functions of `a`.  kappa_p(s) = e^{-s} p!/(2p)! sum_i (p+i)!/(i!(p-i)!) (2s)^{p-i}
    (Rasmussen & Williams, eq. 4.16, with s = sqrt(2 nu) r / l)."""
    x, y = sp.symbols("x y", real=True)
    a, r = sp.symbols("a r", positive=True)

    def kappa(s):
        return sp.Rational(math.factorial(p), math.factorial(2 * p)) * sum(
            sp.Rational(math.factorial(p + i), math.factorial(i) * math.factorial(p - i)) * (2 * s) ** (p - i)
            for i in range(p + 1)) * sp.exp(-s)
    out = []
    for s, sub in ((a * (x - y), {x: y + r}), (a * (y - x), {x: y - r})):
        e = kappa(s)
        for v, n in ((x, n0), (y, n1)):
            if n:
                e = sp.diff(e, v, n)
        q = sp.expand(sp.expand(e.subs(sub)) * sp.exp(a * r))
        assert not q.has(sp.exp) and not q.has(x) and not q.has(y), q
        out.append(sp.Poly(q, r).all_coeffs()[::-1])
    if n0 + n1 <= 2 * p:
        # inside the kernel's differentiability the two one-sided limits at x == y agree
        assert sp.simplify(out[0][0] - out[1][0]) == 0, (p, n0, n1)
    return tuple(sp.lambdify(a, c, "mpmath") for c in out)


@functools.lru_cache(maxsize=None)
def _expquad_poly(n0, n1):
    """d^{n0}_x d^{n1}_y exp(-(x-y)^2 / (2 l^2)) = q(r) exp(-r^2 / (2 l^2)), r = x - y (signed): coefficients of q as a function of l."""
    x, y, r = sp.symbols("x y r", real=True)
    ell = sp.symbols("l", positive=True)
    e = sp.exp(-(x - y) ** 2 / (2 * ell ** 2))
    for v, n in ((x, n0), (y, n1)):
        if n:
            e = sp.diff(e, v, n)
    q = sp.expand(sp.expand(e.subs({x: y + r})) * sp.exp(r ** 2 / (2 * ell ** 2)))
    assert not q.has(sp.exp) and not q.has(x) and not q.has(y), q
    return sp.lambdify(ell, sp.Poly(q, r).all_coeffs()[::-1], "mpmath")


def _horner(c, t):
    acc = mpmath.mpf(0)
    for ck in reversed(c):
        acc = acc * t + ck
    return acc


def _to_ld(v):
    """mpf -> long double as head + tail of the MANTISSA, scaled afterwards: the same value as float(v) + float(v - float(v)) in the
    normal range of float64, and no loss below it (a factor e^{-725} of a scattered pair, tests/_entry_reference.py)."""
    m, e = mpmath.frexp(v)
    hi = float(m)
    return np.ldexp(LD(hi) + LD(float(m - hi)), int(e))


_factor_cache = {}


def factor_matrices(factor, orders, x0, x1):
    """{(n0, n1): (M, E)} for the orders asked: value and envelope of the 1-D factor on x0 (rows) x x1 (columns), long double.
    `factor` = ("matern", nu, lengthscale) | ("expquad", lengthscale), as in `oracle.covfuncs`."""
    x0, x1 = np.asarray(x0, dtype=np.double), np.asarray(x1, dtype=np.double)
    key = (factor, x0.tobytes(), x1.tobytes())
    store = _factor_cache.setdefault(key, {})
    todo = [o for o in orders if o not in store]
    if todo:
        with mpmath.workdps(DPS):
            m0, m1 = [mpmath.mpf(float(v)) for v in x0], [mpmath.mpf(float(v)) for v in x1]
            diff = [[u - v for v in m1] for u in m0]                     # exact
            if factor[0] == "matern":
                p = int(round(factor[1] - 0.5))
                assert abs(p + 0.5 - factor[1]) < 1e-12
                a = mpmath.sqrt(2 * p + 1) / mpmath.mpf(float(factor[2]))
                ex = [[mpmath.exp(-a * abs(t)) for t in row] for row in diff]
                for n0, n1 in todo:
                    assert n0 + n1 <= 2 * p, "beyond the kernel's differentiability"
                    gt, lt = (f(a) for f in _matern_polys(p, n0, n1))
                    agt, alt = [abs(c) for c in gt], [abs(c) for c in lt]
                    M, E = np.empty((len(m0), len(m1)), dtype=LD), np.empty((len(m0), len(m1)), dtype=LD)
                    for i, row in enumerate(diff):
                        for j, t in enumerate(row):
                            c, ca = (gt, agt) if t >= 0 else (lt, alt)
                            M[i, j] = _to_ld(_horner(c, abs(t)) * ex[i][j])
                            E[i, j] = _to_ld(_horner(ca, abs(t)) * ex[i][j])
                    store[(n0, n1)] = (M, E)
            elif factor[0] == "expquad":
                ell = mpmath.mpf(float(factor[1]))
                ex = [[mpmath.exp(-t * t / (2 * ell * ell)) for t in row] for row in diff]
                for n0, n1 in todo:
                    c = _expquad_poly(n0, n1)(ell)
                    ca = [abs(v) for v in c]
                    M, E = np.empty((len(m0), len(m1)), dtype=LD), np.empty((len(m0), len(m1)), dtype=LD)
                    for i, row in enumerate(diff):
                        for j, t in enumerate(row):
                            M[i, j] = _to_ld(_horner(c, t) * ex[i][j])
                            E[i, j] = _to_ld(_horner(ca, abs(t)) * ex[i][j])
                    store[(n0, n1)] = (M, E)
            else:
                raise ValueError(f"unknown factor {factor!r}")
    return {o: store[o] for o in orders}


# ---- the block ----------------------------------------------------------------------------------------------------------------
def grid_block(kernel, L0, L1, F0, F1, flip_dim=None):
    """(G, E) of (L0 k L1) on the tensor grids of the factor coordinates F0 (rows) and F1 (columns), flattened in C order.
    kernel = [(scale, [factor per dimension])], L = {multi-index: coefficient}.
    `flip_dim`: that dimension's factor matrices are taken TRANSPOSED -- evaluated with the roles of x and x' exchanged, which on a
    stationary kernel is M -> (-1)^{n0+n1} M: the wrong block a transposing expansion would write (used to prove that a case sees it)."""
    D = len(F0)
    N0, N1 = int(np.prod([len(f) for f in F0])), int(np.prod([len(f) for f in F1]))
    G, E = np.zeros((N0, N1), dtype=LD), np.zeros((N0, N1), dtype=LD)
    for scale, factors in kernel:
        assert len(factors) == D
        mats = [factor_matrices(tuple(factors[d]), sorted({(a[d], b[d]) for a in L0 for b in L1}), F0[d], F1[d]) for d in range(D)]
        for (a, ca), (b, cb) in itertools.product(L0.items(), L1.items()):
            c = LD(scale) * LD(ca) * LD(cb)
            sign = -1 if flip_dim is not None and (a[flip_dim] + b[flip_dim]) % 2 else 1
            G += (sign * c) * functools.reduce(np.kron, [mats[d][(a[d], b[d])][0] for d in range(D)])
            E += abs(c) * functools.reduce(np.kron, [mats[d][(a[d], b[d])][1] for d in range(D)])
    return G, E


def worst_ratio(got, G, E, mask=None):
    """max over the (masked) entries of |got - G| / E, and its flat position; an entry with E == 0 must be exact."""
    err = np.abs(np.asarray(got).astype(LD) - G)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(E > 0, err / E, np.where(err == 0, LD(0), LD(np.inf)))
    if mask is not None:
        ratio = np.where(mask, ratio, LD(0))
    pos = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[pos]), pos


# ---- which kernel `launch_assemble_kron` picks (csrc/assemble.hip), restated ------------------------------------------------
def distinct_fast(kernel, L0, L1):
    """Number of distinct fast-dimension matrices: keys (group, n0, n1) of the last dimension."""
    return len(kernel) * len({(a[-1], b[-1]) for a in L0 for b in L1})


def selected_kernel(D, nuniq_fast, rows, cols, kron_wide=True):
    if D == 2 and nuniq_fast <= 8 and rows[1] >= 32 and cols[1] >= 16:
        if kron_wide and rows[1] % 2 == 0 and nuniq_fast <= 4:        # (block offsets and the leading dimension are even: 128-padded)
            return "kron2w<4>"
        return "kron2<4>" if nuniq_fast <= 4 else "kron2<8>"
    return f"kron_expand<{D},{2 if nuniq_fast <= 2 else 4 if nuniq_fast <= 4 else 8 if nuniq_fast <= 8 else 16}>"


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# kernels: every dimension has its own family / smoothness / lengthscale, so that two factors of equal extent are not exchangeable
K2 = [(1.3, [("matern", 2.5, 0.9), ("matern", 3.5, 0.7)])]
K2S = K2 + [(0.6, [("expquad", 0.8), ("matern", 2.5, 1.1)])]
K3 = [(1.1, [("matern", 2.5, 0.9), ("expquad", 0.8), ("matern", 3.5, 0.7)])]
K4 = [(0.9, [("matern", 2.5, 0.9), ("expquad", 0.8), ("matern", 1.5, 1.2), ("matern", 3.5, 0.7)])]
# operators {multi-index: coefficient}; each has an ODD order in the fastest dimension (and A* in every dimension)
I2, I3, I4 = {(0, 0): 1.0}, {(0, 0, 0): 1.0}, {(0, 0, 0, 0): 1.0}
A2 = {(0, 0): 0.7, (1, 0): -1.2, (0, 1): 0.9}
B2 = {(0, 0): -0.8, (2, 0): 0.5, (0, 1): 1.1}
G2 = {(0, 0): 0.6, (1, 0): -0.9, (0, 1): 1.2, (2, 0): 0.7, (1, 1): -1.1, (0, 2): 0.8}       # general second order
H2 = {(0, 0): -1.3, (1, 0): 0.8, (0, 1): -0.7, (2, 0): 1.1, (1, 1): 0.9, (0, 2): -0.6}
A3 = {(0, 0, 0): 0.7, (1, 0, 0): -1.2, (0, 1, 0): 0.9, (0, 0, 1): 1.1}
B3 = {(0, 0, 0): -0.8, (0, 2, 0): 0.5, (0, 0, 1): 1.3, (1, 0, 0): 0.6}
C3 = {(0, 0, 0): 0.6, (0, 0, 1): -0.9, (0, 0, 2): 0.7, (1, 0, 0): 1.2, (0, 1, 0): -0.8}
E3 = {(0, 0, 0): -1.1, (0, 0, 1): 0.8, (0, 0, 2): 0.9, (1, 0, 0): -0.7, (0, 1, 0): 1.3}
A4 = {(0, 0, 0, 0): 0.7, (1, 0, 0, 0): -1.2, (0, 1, 0, 0): 0.9, (0, 0, 1, 0): -0.6, (0, 0, 0, 1): 1.1}
B4 = {(0, 0, 0, 0): -0.8, (0, 0, 0, 1): 1.3, (0, 2, 0, 0): 0.5, (0, 0, 1, 0): 0.6}
C4 = {(0, 0, 0, 0): 0.6, (0, 0, 0, 1): -0.9, (0, 0, 0, 2): 0.7, (1, 0, 0, 0): 1.2}
D4 = {(0, 0, 0, 0): -1.1, (0, 0, 0, 1): 0.8, (0, 0, 0, 2): 0.9, (0, 1, 0, 0): -0.7}

# (name, kernel, L0, L1, row extents, column extents, kron_wide)
_SPECS = [
    # D = 2, register-resident kernels: <= 4 distinct fast matrices; the slow pair counts n0s * n1s (off-diagonal) and n0s^2 (diagonal)
    # straddle the KR_PAIRS = 16 chunks: 1, 15, 16, 17, 40 / 1, 9, 64, 289, 25, 16
    ("p1", K2, A2, B2, (1, 34), (1, 16), True),
    ("p15", K2, A2, B2, (3, 34), (5, 33), True),
    ("p16", K2, A2, B2, (8, 34), (2, 70), True),
    ("p17", K2, A2, B2, (17, 34), (1, 16), True),
    ("p40", K2, A2, B2, (5, 130), (8, 33), True),
    ("d16", K2, A2, B2, (4, 130), (3, 70), True),
    ("odd35", K2, A2, B2, (3, 35), (5, 33), True),
    ("odd129", K2, A2, B2, (5, 129), (8, 70), True),
    ("narrow", K2, A2, B2, (4, 34), (3, 16), False),
    ("narrow130", K2, A2, B2, (2, 130), (9, 33), False),
    ("sum8", K2S, A2, B2, (3, 34), (5, 17), True),
    ("sum8b", K2S, A2, B2, (2, 67), (3, 40), True),
    ("six", K2, G2, A2, (4, 66), (3, 33), True),
    # D = 2, the general expansion: short fast dimension (columns 1, 3, 7, 8, 9, 15, 17; rows < 32), or more than 8 fast matrices
    ("c1", K2, A2, I2, (9, 7), (11, 1), True),
    ("c3", K2, A2, I2, (5, 31), (7, 3), True),
    ("c8", K2, A2, B2, (6, 17), (10, 8), True),
    ("c9", K2, A2, B2, (12, 3), (5, 9), True),
    ("c15", K2, A2, B2, (3, 40), (4, 15), True),
    ("c17", K2, G2, A2, (7, 15), (3, 17), True),
    ("c7", K2, G2, H2, (9, 15), (6, 7), True),
    ("wide9", K2, G2, H2, (3, 36), (4, 17), True),
    ("r1", K2, A2, I2, (70, 1), (33, 1), True),
    # D = 3
    ("t", K3, A3, I3, (3, 5, 7), (2, 4, 9), True),
    ("t-slow1", K3, A3, B3, (5, 1, 17), (3, 2, 8), True),
    ("t-fastrow1", K3, A3, B3, (9, 8, 1), (7, 5, 2), True),
    ("t-fastcol1", K3, A3, B3, (6, 5, 3), (8, 9, 1), True),
    ("t-big", K3, A3, B3, (6, 7, 9), (5, 4, 17), True),
    ("t-six", K3, C3, A3, (7, 3, 11), (5, 2, 33), True),
    ("t-nine", K3, C3, E3, (4, 5, 9), (3, 7, 15), True),
    # D = 4
    ("q", K4, A4, I4, (3, 2, 4, 5), (2, 3, 5, 7), True),
    ("q-slow1", K4, A4, B4, (4, 3, 1, 9), (3, 2, 2, 17), True),
    ("q-fastrow1", K4, A4, B4, (3, 4, 5, 1), (2, 3, 4, 3), True),
    ("q-fastcol1", K4, A4, B4, (2, 3, 4, 3), (3, 4, 5, 1), True),
    ("q-six", K4, C4, A4, (3, 2, 5, 8), (2, 3, 4, 15), True),
    ("q-nine", K4, C4, D4, (2, 3, 2, 9), (3, 2, 3, 7), True),
]


class Case:
    """One block: `kind` "off" = rows grid x columns grid, "diag" = the rows grid against itself (lower triangle)."""

    def __init__(self, name, kernel, L0, L1, rows, cols, kron_wide, kind):
        self.name, self.kernel, self.L0, self.L1, self.kron_wide, self.kind = name, kernel, L0, L1, kron_wide, kind
        self.rows = tuple(rows)
        self.cols = tuple(cols) if kind == "off" else self.rows
        self.D = len(rows)
        self.nuniq = distinct_fast(kernel, L0, L1)
        self.kernel_name = selected_kernel(self.D, self.nuniq, self.rows, self.cols, kron_wide)
        self.id = f"{self.kernel_name}-{kind}-{name}" + ("" if kron_wide else "-nowide")
        # sorted random coordinates, a seed of its own per (case, side, dimension): NOT equispaced, so no factor is Toeplitz
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
        self.F0 = [np.sort(np.random.default_rng([seed, 0, d]).uniform(0.0, 1.5, n)) for d, n in enumerate(self.rows)]
        self.F1 = ([np.sort(np.random.default_rng([seed, 1, d]).uniform(0.0, 1.5, n)) for d, n in enumerate(self.cols)]
                   if kind == "off" else self.F0)

    @property
    def shape(self):
        return int(np.prod(self.rows)), int(np.prod(self.cols))

    def reference(self, flip_dim=None):
        return grid_block(self.kernel, self.L0, self.L1, self.F0, self.F1, flip_dim)

    def mask(self):
        """The entries the assembly is supposed to write."""
        n0, n1 = self.shape
        return np.ones((n0, n1), dtype=bool) if self.kind == "off" else np.tril(np.ones((n0, n1), dtype=bool))

    def flip_dim(self):
        """The dimension whose transposition the case must see: the fastest one in which the block has more than one distinct
        (x, x') pair class -- on a diagonal block a dimension of extent 1 only has x == x', where transposing changes nothing."""
        for d in range(self.D - 1, -1, -1):
            if self.kind == "off" or self.rows[d] > 1:
                return d
        raise AssertionError("a one-point block")

    def describe(self, pos):
        n1 = self.shape[1]
        return (tuple(int(v) for v in np.unravel_index(pos // n1, self.rows)),
                tuple(int(v) for v in np.unravel_index(pos % n1, self.cols)))

    def mesh(self):
        """(X0, X1): the flattened C-order meshes."""
        f = lambda F: np.stack(np.meshgrid(*F, indexing="ij"), axis=-1).reshape(-1, len(F))
        return f(self.F0), f(self.F1)


CASES = [Case(*spec, kind) for spec in _SPECS for kind in ("off", "diag")]
