"""High-precision reference of one block of (L0 k L1'^*)(X0, X1) on SCATTERED points, its entry bound, and the case list of the
entry-exact suites of the per-entry evaluation core (test_entry_reference.py on the CPU, test_gpu_entry_exact.py on the device).
A plain module, not a conftest.

The block.  kernel = [(scale, [factor per dimension])], L = {multi-index: coefficient}, as in `_kron_reference`.  The 1-D factors
d^{n0}/dx^{n0} d^{n1}/dx'^{n1} k_d are `_kron_reference.factor_matrices` (SymPy closed form, mpmath at 34 digits, exact binary
coordinates) on the coordinate columns X0[:, d], X1[:, d]; a scattered block combines them ELEMENTWISE,
    G_ij = sum_g scale_g sum_t c_t prod_d M_{g,t,d}[i, j],        E_ij = sum_g |scale_g| sum_t |c_t| prod_d E_{g,t,d}[i, j],
in `np.longdouble`.  E is the envelope: the same expression with every polynomial coefficient absolute.

The bound.  With r_d = a_d |x_d - x'_d| (a_d = sqrt(2 nu) / l for a Matern dimension, 1 / l for a squared-exponential one) the device
evaluates exp(-(sum_Matern r_d + sum_ExpQuad r_d^2 / 2)).  The roundings of x - x', of a_d and of the product are RELATIVE errors of
r_d, i.e. an absolute error of about rho eps in the exponent,
    rho_g = sum_d (r_d for a Matern dimension, r_d^2 for a squared-exponential one),
which does not stay a fixed multiple of E as the points move apart (the radial suite met it at s ~ 50).  So an entry is held to
    |got - G| <= K * W + eta,        W = sum_g (1 + rho_g) E_g
(for one group W = (1 + rho) E; for a sum every group carries its own rho), K measured, not chosen: see K_ENTRY below.

eta: gradual underflow.  The last line of `eval_entries` (csrc/eval_entries.h) and of `fast_entries` (csrc/assemble.hip) is
    res = fma(scale * lpgp_exp_neg(expo), tot, res)
with tot the signed sum of the Horner chains, |tot| <= P (1 + O(eps)), P = E_g / (|scale_g| e^{-expo}) the polynomial envelope
without its exponential.  Where e^{-expo} < 2^-1022 three roundings land on the subnormal grid of spacing 2^-1074 and are
ABSOLUTE errors of at most 2^-1075 each, whatever the magnitude of the value:
    x = lpgp_exp_neg(expo)   (its final ldexp)          |x - e^{-expo}(1 + O(eps))| <= 2^-1075
    y = fl(scale * x)                                    |y - scale x|               <= 2^-1075
    res = fl(y * tot + res)                              the fma's own rounding      <= 2^-1075
so the entry moves by at most (|scale| 2^-1075 + 2^-1075) |tot| + 2^-1075:
    eta_g = 2^-1075 ((|scale_g| + 1) P_g + 1)     where  min(1, |scale_g|) e^{-expo} < 2^-1021,     0 elsewhere
-- P may be 1e11 (a bi-Laplacian at r = 700), so this is not "an ulp": it is eleven orders above the subnormal spacing.  The window
is taken one binade wide of 2^-1022 (and includes y going subnormal under |scale| < 1) because the device's expo is the rounded
one.  For |scale| P >= P + 1 this is below the 2^-1074 |scale| P one would write down without the fma's own rounding.  Beyond the
clamp of lpgp_exp_neg (expo > 800: e^{-800} ~ 1e-348) the device writes exactly +-0, and |0 - G| <= eta there by the same count.

The isotropic first-order group (DevGroup::iso == 1) has its reference in tests/golden/iso_first.npz (50-digit SymPy / mpmath blocks
with the all-summands-absolute envelope, made by tests/golden/make_golden_iso_radial.py): `iso_first_cases()`; rho = s there.

K (measured on the CPU by test_entry_reference.py, which asserts that these are the values):
    K_ENTRY     = max(4 max_cases max_ij |oracle.covfuncs.LkL - G| / W, 8 eps)
    K_ISO_FIRST = max(4 max_cases max_ij |_iso_radial_reference.block - G| / ((1 + s) E), 8 eps)
The oracle / the helper are plain NumPy float64 evaluations of the same closed forms; the factor 4 is the one this project has used
for the Kronecker and the radial suites: the device sums merged coefficients in another order, multiplies rounded factors and uses
the table exponential.  Neither K is ever raised to make a device run pass."""
import math
import os

import numpy as np

import _kron_reference as kr

LD = kr.LD
EPS = kr.EPS
SUB = LD(2) ** -1075                 # half the subnormal spacing of float64
WINDOW = LD(2) ** -1021
EXP_CLAMP = 800.0                    # lpgp_exp_neg (csrc/eval_entries.h)
MAX_ENTRIES = 20000                  # per case: ~26 us per mpmath factor entry

# Measured by test_entry_reference.py::test_reference_against_the_oracle / ::test_iso_first_helper_against_the_golden (they print
# the ratio per case and assert these figures); MEASUREMENTS.md, "Entry-exact scattered assembly and matrix-free product".
RHO_ORACLE_MAX = 3.71 * EPS          # set by assemble_fast<2,3,3,0>-s2-q33-odd-off130x17-a at (68, 15), rho = 0.119
K_ENTRY = max(4 * RHO_ORACLE_MAX, 8 * EPS)
RHO_HELPER_MAX = 5.73 * EPS          # set by d2_nu72-id_grad at (8, 8): a pair 1e-5 of a lengthscale apart (s = 2.6e-5)
K_ISO_FIRST = max(4 * RHO_HELPER_MAX, 8 * EPS)


def scales(factors):
    """a_d of every dimension, in float64 as the lowering forms them."""
    return [math.sqrt(2.0 * f[1]) / f[2] if f[0] == "matern" else 1.0 / f[1] for f in factors]


def exponent_and_rho(factors, X0, X1):
    """(expo, rho) of one group in long double: the exponent of its exponential and the weight of the argument's rounding."""
    expo = np.zeros((X0.shape[0], X1.shape[0]), dtype=LD)
    rho = np.zeros_like(expo)
    for d, (f, a) in enumerate(zip(factors, scales(factors))):
        r = LD(a) * np.abs(X0[:, None, d].astype(LD) - X1[None, :, d].astype(LD))
        if f[0] == "matern":
            expo += r
            rho += r
        else:
            expo += r * r / 2
            rho += r * r
    return expo, rho


class Block:
    """G, E, W = sum_g (1 + rho_g) E_g, eta, rho = max_g rho_g, expo = min_g expo_g, expo0 = the first group's exponent (all n0 x n1,
    long double)."""

    def __init__(self, G, E, W, eta, rho, expo, expo0=None):
        self.G, self.E, self.W, self.eta, self.rho, self.expo = G, E, W, eta, rho, expo
        self.expo0 = expo if expo0 is None else expo0

    def bound(self, K):
        return LD(K) * self.W + self.eta

    def ratio(self, got, mask=None):
        """max over the (masked) entries of max(|got - G| - eta, 0) / W and its flat position; where W == 0 the entry must be
        within eta."""
        err = np.maximum(np.abs(np.asarray(got).astype(LD) - self.G) - self.eta, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(self.W > 0, err / self.W, np.where(err == 0, LD(0), LD(np.inf)))
        if mask is not None:
            ratio = np.where(mask, ratio, LD(0))
        pos = int(np.argmax(ratio))
        return float(ratio.reshape(-1)[pos]), pos


def scattered_block(kernel, L0, L1, X0, X1, plus_dim=None, flip_dim=None, roll=False):
    """The reference block.  The wrong blocks a broken kernel would write (used to prove that a case sees them):
    `plus_dim`: that dimension's sign forced to +1 -- every factor of odd order there evaluated on its x > x' branch;
    `flip_dim`: rows and columns exchanged in that dimension, x_d - x'_d -> x'_d - x_d: on a stationary kernel (-1)^{n0+n1} M;
    `roll`: the fastest dimension's factor taken one column to the side (one row, on a block of one column)."""
    X0, X1 = np.asarray(X0, dtype=np.double), np.asarray(X1, dtype=np.double)
    D = X0.shape[1]
    n0, n1 = X0.shape[0], X1.shape[0]
    assert n0 * n1 <= MAX_ENTRIES
    G, E, W, eta = (np.zeros((n0, n1), dtype=LD) for _ in range(4))
    rho_max = np.zeros((n0, n1), dtype=LD)
    expo_min = np.full((n0, n1), np.inf, dtype=LD)
    expo0 = None
    for scale, factors in kernel:
        assert len(factors) == D
        mats = [kr.factor_matrices(tuple(factors[d]), sorted({(a[d], b[d]) for a in L0 for b in L1}), X0[:, d], X1[:, d]) for d in range(D)]
        Gg, Eg = np.zeros((n0, n1), dtype=LD), np.zeros((n0, n1), dtype=LD)
        for a, ca in L0.items():
            for b, cb in L1.items():
                c = LD(scale) * LD(ca) * LD(cb)
                m, e = LD(1), LD(1)
                for d in range(D):
                    Md, Ed = mats[d][(a[d], b[d])]
                    odd = (a[d] + b[d]) % 2 == 1
                    if odd and d == plus_dim:
                        Md = Md * np.sign(X0[:, None, d] - X1[None, :, d])
                    if odd and d == flip_dim:
                        Md = -Md
                    if roll and d == D - 1:
                        Md = np.roll(Md, 1, axis=1 if n1 > 1 else 0)
                    m, e = m * Md, e * Ed
                Gg += c * m
                Eg += abs(c) * e
        expo, rho = exponent_and_rho(factors, X0, X1)
        ex = np.exp(-expo)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            P = np.where(ex > 0, Eg / (abs(LD(scale)) * ex), LD(0)) if scale != 0 else np.zeros_like(Eg)
        eta += np.where(min(1.0, abs(scale)) * ex < WINDOW, SUB * ((abs(LD(scale)) + 1) * P + 1), LD(0))
        G += Gg
        E += Eg
        W += (1 + rho) * Eg
        rho_max = np.maximum(rho_max, rho)
        expo_min = np.minimum(expo_min, expo)
        expo0 = expo if expo0 is None else expo0
    return Block(G, E, W, eta, rho_max, expo_min, expo0)


# ---- which kernel the host picks (csrc/assemble.hip: fast_shape, fast_mode, asm_flags), restated -------------------------------
def fast_instantiation(kernel, L0, L1):
    """(N0, N1, MODE) of `assemble_fast_kernel<D, N0, N1, MODE>` / `matvec_fast_kernel`, or None where `fast_shape` refuses: D <= 2,
    one product-form group, at most two parity classes, N = degree + 1 <= 5 per dimension, classes * N0 * N1 <= 32.
    The degree in r_d: nu - 1/2 for a Matern dimension (differentiating P(r) e^{-r} keeps the degree), the largest derivative
    order for a squared-exponential one (a Hermite polynomial).  A parity class is the vector of (n0 + n1) mod 2 over the
    dimensions.  MODE 0: some dimension is squared-exponential; 1: all Matern, some class flips a sign; 2: all Matern, all even."""
    D = len(next(iter(L0)))
    if D > 2 or len(kernel) != 1:
        return None
    factors = kernel[0][1]
    classes = {tuple((a[d] + b[d]) % 2 for d in range(D)) for a in L0 for b in L1}
    deg = [int(round(f[1] - 0.5)) if f[0] == "matern" else max(a[d] + b[d] for a in L0 for b in L1) for d, f in enumerate(factors)]
    N0, N1 = deg[0] + 1, (deg[1] + 1 if D > 1 else 1)
    if len(classes) > 2 or N0 > 5 or N1 > 5 or len(classes) * N0 * N1 > 32:
        return None
    if any(f[0] != "matern" for f in factors):
        return N0, N1, 0
    return N0, N1, (1 if any(any(c) for c in classes) else 2)


def kernel_name(kernel, L0, L1, factors=False, product=False):
    """The instantiation a launch with this descriptor runs.  `factors`: `asm_factors = 1` (at most FACT_MAXG = 4 groups) sends
    every product-form descriptor to the generic kernel with per-point exponential factors."""
    D = len(next(iter(L0)))
    fast = None if factors else fast_instantiation(kernel, L0, L1)
    stem = "matvec" if product else "assemble"
    if fast is not None:
        return f"{stem}_fast<{D},{fast[0]},{fast[1]},{fast[2]}>"
    return f"{stem}<{D},{'F' if factors else '-'}>"


def all_matern(kernel):
    return all(f[0] == "matern" for _, factors in kernel for f in factors)


# ---- descriptors -------------------------------------------------------------------------------------------------------------
# every dimension has its own family / smoothness / lengthscale; the operators have an odd order in the FASTEST dimension wherever
# the instantiation allows one (MODE 2 is defined by having none; nu = 1/2 admits no derivative)
M = lambda nu, l: ("matern", nu, l)      # noqa: E731
Q = lambda l: ("expquad", l)             # noqa: E731
LAP2 = {(0, 0): 0.3, (2, 0): 1.0, (0, 2): 1.0}
DESCRIPTORS = {
    # specialised, D = 1 (N1 = 1)
    "s1-q5": ([(1.2, [Q(0.8)])], {(0,): 0.7, (1,): -1.2, (2,): 0.5}, {(0,): -0.8, (1,): 1.1, (2,): 0.6}),          # MODE 0, N0 = 5
    "s1-q1": ([(0.9, [Q(1.1)])], {(0,): 1.0}, {(0,): 1.0}),                                                        # MODE 0, N0 = 1
    "s1-m3": ([(1.3, [M(2.5, 0.9)])], {(0,): 0.7, (1,): -1.2}, {(0,): 1.0}),                                      # MODE 1, N0 = 3
    "s1-m5": ([(1.1, [M(4.5, 1.2)])], {(0,): 1.0}, {(0,): 1.0}),                                                   # MODE 2, N0 = 5
    "s1-m1": ([(0.8, [M(0.5, 0.7)])], {(0,): 1.0}, {(0,): 1.0}),                                                   # MODE 2, N0 = 1
    # specialised, D = 2
    "s2-13-odd": ([(1.3, [M(0.5, 0.9), M(2.5, 0.7)])], {(0, 0): 0.7, (0, 1): 0.9}, {(0, 0): 1.0}),                 # MODE 1 <1,3>
    "s2-51-odd": ([(0.7, [M(4.5, 1.1), M(0.5, 0.8)])], {(0, 0): 0.7, (1, 0): -1.2}, {(0, 0): 1.0}),                # MODE 1 <5,1> (nu = 1/2 fastest)
    "s2-35-odd": ([(1.2, [M(2.5, 0.9), M(4.5, 1.3)])], {(0, 0): 0.7, (0, 1): 0.9}, {(0, 0): -0.8, (2, 0): 0.5}),   # MODE 1 <3,5>
    "s2-53-lap": ([(1.1, [M(4.5, 1.2), M(2.5, 0.8)])], LAP2, {(0, 0): 1.0}),                                       # MODE 2 <5,3>
    "s2-33-laplap": ([(0.9, [M(2.5, 0.9), M(2.5, 0.6)])], LAP2, {(0, 0): -0.4, (2, 0): 0.8, (0, 2): 1.1}),         # MODE 2 <3,3>
    "s2-15": ([(1.4, [M(0.5, 0.8), M(4.5, 1.1)])], {(0, 0): 1.0}, {(0, 0): 1.0}),                                  # MODE 2 <1,5>
    "s2-11": ([(0.6, [M(0.5, 0.8), M(0.5, 1.3)])], {(0, 0): 1.0}, {(0, 0): 1.0}),                                  # MODE 2 <1,1>
    "s2-q33-odd": ([(1.2, [Q(0.8), M(2.5, 0.7)])], {(0, 0): 0.7, (0, 1): 0.9}, {(0, 0): -0.8, (2, 0): 0.5}),       # MODE 0 <3,3>
    "s2-5q3-odd": ([(0.8, [M(4.5, 1.1), Q(0.9)])], {(0, 0): 0.7, (0, 1): 0.9}, {(0, 0): -0.8, (0, 1): 1.1}),       # MODE 0 <5,3>
    # generic
    "g2-sum": (kr.K2S, kr.A2, kr.B2),                 # a sum of two groups
    "g2-classes": (kr.K2, kr.G2, kr.H2),              # general second order on both sides: four parity classes
    "g3": (kr.K3, kr.A3, kr.B3),
    "g4": (kr.K4, kr.A4, kr.B4),
}
EXPECTED = {
    "s1-q5": "assemble_fast<1,5,1,0>", "s1-q1": "assemble_fast<1,1,1,0>", "s1-m3": "assemble_fast<1,3,1,1>",
    "s1-m5": "assemble_fast<1,5,1,2>", "s1-m1": "assemble_fast<1,1,1,2>",
    "s2-13-odd": "assemble_fast<2,1,3,1>", "s2-51-odd": "assemble_fast<2,5,1,1>", "s2-35-odd": "assemble_fast<2,3,5,1>",
    "s2-53-lap": "assemble_fast<2,5,3,2>", "s2-33-laplap": "assemble_fast<2,3,3,2>", "s2-15": "assemble_fast<2,1,5,2>",
    "s2-11": "assemble_fast<2,1,1,2>", "s2-q33-odd": "assemble_fast<2,3,3,0>", "s2-5q3-odd": "assemble_fast<2,5,3,0>",
    "g2-sum": "assemble<2,->", "g2-classes": "assemble<2,->", "g3": "assemble<3,->", "g4": "assemble<4,->",
}

# ---- point sets ----------------------------------------------------------------------------------------------------------------
PLANT = 12                  # planted pairs occupy the first PLANT points of a side
T_NEAR, T_FAR, T_SUB, T_ZERO = 50.0, 650.0, 725.0, 850.0      # exponents of the planted far pairs


def _lengths(kernel):
    """Per dimension: (lengthscale, distance per unit of the exponent's share t_d: r_d = t_d or r_d^2 / 2 = t_d) of the FIRST group."""
    out = []
    for f, a in zip(kernel[0][1], scales(kernel[0][1])):
        out.append((f[-1], (lambda t, a=a: t / a) if f[0] == "matern" else (lambda t, a=a: math.sqrt(2 * t) / a)))
    return out


def _plant(kernel, base, rng):
    """12 partners of the points `base[:12]`: 0 coincident; 1 equal in dimension 0 only; 2, 3 at 1e-9 / 1e-5 of a lengthscale; 4, 5 at
    exponent ~ 50; 6, 7 at ~ 650 (still normal); 8 in the subnormal window (725); 9 beyond the clamp (850); 10, 11 left scattered."""
    D = base.shape[1]
    ls = _lengths(kernel)
    out = rng.uniform(0.0, 3.0, (PLANT, D))
    out[0] = base[0]
    if D > 1:
        out[1, 0] = base[1, 0]
    for i, eps in ((2, 1e-9), (3, 1e-5)):
        e = rng.normal(size=D)
        out[i] = base[i] + eps * np.array([l for l, _ in ls]) * e / np.linalg.norm(e)
    for i, t in ((4, T_NEAR), (5, T_NEAR), (6, T_FAR), (7, T_FAR), (8, T_SUB), (9, T_ZERO)):
        share = rng.dirichlet(np.full(D, 4.0)) * t                       # the exponent, split over the dimensions
        sign = rng.choice([-1.0, 1.0], size=D)
        out[i] = base[i] + sign * np.array([dist(s) for (_, dist), s in zip(ls, share)])
    return out


def _clusters(n, rng, D, spec):
    """Set (c): points dealt to 64-point tiles; tile k is uniform in a box of `width` lengthscale units at `centre` (units of 1)."""
    X = np.empty((n, D))
    for k in range((n + 63) // 64):
        centre, width = spec[k % len(spec)]
        m = min(64, n - 64 * k)
        X[64 * k: 64 * k + m] = centre + rng.uniform(0.0, width, (m, D))
    return X


def points(name, kernel, D, kind, n0, n1, pset):
    """(X0, X1) of a case; X1 is X0 for a diagonal block.  One seed per case and side."""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(f"{name}-{kind}-{n0}-{n1}-{pset}"))
    r0, r1 = np.random.default_rng([seed, 0]), np.random.default_rng([seed, 1])
    if pset == "c":
        # rows: a tight tile, a tile spread over 40 lengthscales (beyond FACT_TMAX of its origin), a tight tile 300 away
        X0 = _clusters(n0, r0, D, [(0.0, 3.0), (1.0, 40.0), (300.0, 3.0)])
        X1 = X0 if kind == "diag" else _clusters(n1, r1, D, [(0.5, 3.0), (300.5, 3.0), (2.0, 40.0)])
        return X0, X1
    X0 = r0.uniform(0.0, 3.0, (n0, D))
    X1 = X0 if kind == "diag" else r1.uniform(0.0, 3.0, (n1, D))
    if pset == "b":
        if kind == "diag":
            assert n0 >= 2 * PLANT
            X0[PLANT:2 * PLANT] = _plant(kernel, X0[:PLANT], r1)        # entries (12 + k, k): inside the lower triangle
        else:
            assert n0 >= PLANT and n1 >= PLANT
            X1[:PLANT] = _plant(kernel, X0[:PLANT], r1)
    return X0, X1


def factor_tiles(kernel, X0, X1, lower=False):
    """(passing, falling back) 64 x 64 tiles of `assemble_kernel<D, true>` on this block, restated from stage_factors: a tile keeps
    its per-point factors iff |a_d (x_d - origin_d)| <= FACT_TMAX = 32 for every Matern dimension of every group and every valid row
    and column point of the tile, the origin being the tile's first column point.  Tiles within 1 of the threshold count as neither."""
    ok = bad = 0
    for tr in range(0, X0.shape[0], 64):
        for tc in range(0, X1.shape[0], 64):
            if lower and tc > tr:
                continue                     # (a diagonal block: tiles above the diagonal are not evaluated)
            pts = np.concatenate([X0[tr:tr + 64], X1[tc:tc + 64]]) - X1[tc]
            worst = max(abs(a * pts[:, d]).max() for _, factors in kernel for d, (f, a) in enumerate(zip(factors, scales(factors)))
                        if f[0] == "matern")
            ok += worst <= 31.0
            bad += worst >= 33.0
    return int(ok), int(bad)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, desc, kind, n0, n1, pset):
        self.desc, self.kind, self.pset = desc, kind, pset
        self.kernel, self.L0, self.L1 = DESCRIPTORS[desc]
        self.D = len(next(iter(self.L0)))
        self.n0, self.n1 = n0, (n1 if kind == "off" else n0)
        self.expected = EXPECTED[desc]
        self.id = f"{self.expected}-{desc}-{kind}{self.n0}x{self.n1}-{pset}"
        self._pts = self._ref = None

    def points(self):
        if self._pts is None:
            self._pts = points(self.desc, self.kernel, self.D, self.kind, self.n0, self.n1, self.pset)
        return self._pts

    def reference(self, **wrong):
        X0, X1 = self.points()
        if wrong:
            return scattered_block(self.kernel, self.L0, self.L1, X0, X1, **wrong)
        if self._ref is None:
            self._ref = scattered_block(self.kernel, self.L0, self.L1, X0, X1)
        return self._ref

    def mask(self):
        m = np.ones((self.n0, self.n1), dtype=bool)
        return m if self.kind == "off" else np.tril(m)

    def odd_dims(self):
        return [d for d in range(self.D) if any((a[d] + b[d]) % 2 for a in self.L0 for b in self.L1)]

    @property
    def factored(self):
        """Also run with `asm_factors = 1`: product-form Matern descriptors on the sets (a) and (c)."""
        return all_matern(self.kernel) and self.pset in ("a", "c")


def _cases():
    out = []
    full = ("s2-35-odd", "g2-sum")          # every shape on the sets (a) and (b), on one specialised and one generic descriptor
    diag = full + ("s1-m3", "s2-q33-odd", "g3", "g4")
    for desc in DESCRIPTORS:
        if desc in full:
            out.append(Case(desc, "off", 1, 1, "a"))
            for pset in ("a", "b"):
                out += [Case(desc, "off", 64, 64, pset), Case(desc, "off", 65, 150, pset), Case(desc, "off", 130, 17, pset),
                        Case(desc, "diag", 130, 130, pset)]
            out += [Case(desc, "off", 130, 150, "c"), Case(desc, "diag", 130, 130, "c")]
        else:
            # the ragged off-diagonal block with planted pairs, the tall one on plain points; Matern products also on set (c)
            out += [Case(desc, "off", 65, 150, "b"), Case(desc, "off", 130, 17, "a")]
            if desc in diag:
                out.append(Case(desc, "diag", 130, 130, "a"))
            if all_matern(DESCRIPTORS[desc][0]):
                out.append(Case(desc, "off", 130, 70, "c"))
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)


# ---- the isotropic first-order group -------------------------------------------------------------------------------------------
ISO_OPS = ("id_id", "grad_id", "id_grad", "grad_grad", "mix")


def iso_first_pairs(d, v, w, c):
    z = (0,) * d
    e = lambda i: tuple(1 if j == i else 0 for j in range(d))       # noqa: E731
    ident = {z: 1.0}
    gv, gw = {e(i): float(v[i]) for i in range(d)}, {e(i): float(w[i]) for i in range(d)}
    mix = dict(gv)
    mix[z] = float(c)
    return {"id_id": (ident, ident), "grad_id": (gv, ident), "id_grad": (ident, gw), "grad_grad": (gv, gw), "mix": (mix, mix)}


_golden = None


def iso_first_cases():
    """[(id, d, p, lengthscales, L0, L1, X0, X1, Block)] of tests/golden/iso_first.npz; W = (1 + s) E, eta by the count above with the
    polynomial envelope E e^{s}."""
    global _golden
    if _golden is not None:
        return _golden
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iso_first.npz"))
    out = []
    for d in (2, 3):
        for p in (0, 1, 2, 3):
            tag = f"d{d}_nu{2 * p + 1}2"
            ls, X0, X1 = z[tag + "_lengthscales"], z[tag + "_X0"], z[tag + "_X1"]
            a = math.sqrt(2 * p + 1) / ls
            u = LD(1) * a * (X0[:, None, :].astype(LD) - X1[None, :, :].astype(LD))
            s = np.sqrt(np.sum(u * u, axis=-1))
            for name, (L0, L1) in iso_first_pairs(d, z[tag + "_v"], z[tag + "_w"], z[tag + "_c"]).items():
                if f"{tag}_{name}" not in z.files:         # nu = 1/2: id_id only; nu = 3/2: no derivative on both arguments
                    assert p < 2
                    continue
                G, E = z[f"{tag}_{name}"].astype(LD), z[f"{tag}_{name}_E"].astype(LD)
                ex = np.exp(-s)
                eta = np.where(ex < WINDOW, SUB * (2 * E / ex + 1), LD(0))          # (scale = 1; no pair of the file is that far)
                out.append((f"{tag}-{name}", d, p, ls, L0, L1, X0, X1, Block(G, E, (1 + s) * E, eta, s, s)))
    _golden = out
    return out


def iso_first_block(p, lengthscales, L0, L1, X0, X1, scale=1.0):
    """The isotropic first-order block on ANY points (the matrix-free product cases), mpmath at 34 digits on the exact coordinates:
    with u = a .* (x - x'), s = |u|, psi(s^2 / 2) = kappa(s), psi^(m) = e^{-s} Theta_m(s)  (Theta_m: `_iso_radial_reference.theta`,
    rational), L0 = c0 + <v, grad>, L1 = c1 + <w, grad'>, d/dx_i = a_i d/du_i, d/dx'_i = -a_i d/du_i:
        G = c0 c1 psi + (c1 sum_i v_i a_i u_i - c0 sum_j w_j a_j u_j) psi' - sum_ij v_i a_i w_j a_j (psi'' u_i u_j + [i == j] psi')
    E: every summand -- per i, per (i, j), per power of s in Theta_m -- absolute.  test_entry_reference.py holds it to the SymPy
    blocks of tests/golden/iso_first.npz on that file's points."""
    import mpmath
    from _iso_radial_reference import theta
    X0, X1 = np.asarray(X0, dtype=np.double), np.asarray(X1, dtype=np.double)
    d = X0.shape[1]
    assert X0.shape[0] * X1.shape[0] <= MAX_ENTRIES
    z = (0,) * d
    e = lambda i: tuple(1 if j == i else 0 for j in range(d))       # noqa: E731
    assert all(sum(k) <= 1 for k in list(L0) + list(L1))
    n0, n1 = X0.shape[0], X1.shape[0]
    G, E, S = (np.zeros((n0, n1), dtype=LD) for _ in range(3))
    with mpmath.workdps(kr.DPS):
        a = [mpmath.sqrt(2 * p + 1) / mpmath.mpf(float(l)) for l in np.broadcast_to(lengthscales, (d,))]
        th = [[(k, mpmath.mpf(c.numerator) / c.denominator) for k, c in t.items()] for t in theta(p)[:3]]
        c0, c1 = mpmath.mpf(float(L0.get(z, 0.0))), mpmath.mpf(float(L1.get(z, 0.0)))
        v = [mpmath.mpf(float(L0.get(e(i), 0.0))) * a[i] for i in range(d)]
        w = [mpmath.mpf(float(L1.get(e(i), 0.0))) * a[i] for i in range(d)]
        m0, m1 = [[mpmath.mpf(float(x)) for x in row] for row in X0], [[mpmath.mpf(float(x)) for x in row] for row in X1]
        for i in range(n0):
            for j in range(n1):
                u = [a[k] * (m0[i][k] - m1[j][k]) for k in range(d)]
                s = mpmath.sqrt(sum(x * x for x in u))
                ex = mpmath.exp(-s)
                # coefficient (signed, absolute) of psi^(m): [m] -> list of (value, |value| of each summand added up)
                co = [(c0 * c1, abs(c0 * c1)),
                      (sum(c1 * v[k] * u[k] - c0 * w[k] * u[k] - v[k] * w[k] for k in range(d)),
                       sum(abs(c1 * v[k] * u[k]) + abs(c0 * w[k] * u[k]) + abs(v[k] * w[k]) for k in range(d))),
                      (-sum(v[k] * u[k] * w[l] * u[l] for k in range(d) for l in range(d)),
                       sum(abs(v[k] * u[k] * w[l] * u[l]) for k in range(d) for l in range(d)))]
                g = en = mpmath.mpf(0)
                for m, (cv, ca) in enumerate(co):
                    if ca == 0:
                        continue
                    for pw, t in th[m]:
                        if pw < 0 and s == 0:
                            assert cv == 0      # (a negative power only meets u_i u_j)
                            continue
                        g += cv * t * s ** pw * ex
                        en += ca * abs(t) * s ** pw * ex
                G[i, j], E[i, j], S[i, j] = kr._to_ld(g), kr._to_ld(en), kr._to_ld(s)
    sc = LD(scale)
    ex = np.exp(-S)
    eta = np.where(min(1.0, abs(scale)) * ex < WINDOW, SUB * ((abs(sc) + 1) * E / ex + 1), LD(0))
    return Block(sc * G, abs(sc) * E, (1 + S) * abs(sc) * E, eta, S, S)


# ---- the matrix-free product ---------------------------------------------------------------------------------------------------
def product_depth(per, splits, accumulate):
    """The length of the longest chain of additions behind one output of `matvec_kernel` / `matvec_fast_kernel` + `mv_reduce_kernel`
    (csrc/assemble.hip), restated: a thread fuses its 16 columns of every one of the `per` column tiles of its split into y (16 fma
    per tile), wave 0 adds the three other waves' partial sums, the reduction adds `splits` partial sums, `accumulate` one more."""
    return 16 * per + 3 + splits + (1 if accumulate else 0)


def split_plan(n0, n1, cus):
    """(tiles_r, tiles_c, splits, per, tiles owned by each split) as `lpgp_kernel_matvec` (csrc/api.hip) and the kernels form them."""
    tiles_r, tiles_c = (n0 + 63) // 64, (n1 + 63) // 64
    splits = max(1, min((4 * cus + tiles_r - 1) // tiles_r, tiles_c))
    per = (tiles_c + splits - 1) // splits
    owned = [max(0, min((sp + 1) * per, tiles_c) - sp * per) for sp in range(splits)]
    return tiles_r, tiles_c, splits, per, owned


def product_reference(block, V, K, per, splits, accumulate=False, old=None):
    """(y, bound) per row and right-hand side, long double: y = sum_j G_ij v_j (+ old), bound = sum_j B_ij |v_j| + depth u (sum_j E_ij
    |v_j| + |old|), B the entry bound, u = 2^-53."""
    Va = np.abs(V).astype(LD)
    y = block.G @ V.astype(LD)
    env = block.E @ Va
    if accumulate:
        y = y + old.astype(LD)
        env = env + np.abs(old).astype(LD)
    return y, block.bound(K) @ Va + product_depth(per, splits, accumulate) * LD(EPS) * env


DESCRIPTORS["g2-sum-lite"] = (kr.K2S, {(0, 0): 0.7, (0, 1): 0.9}, {(0, 0): 1.0})
EXPECTED["g2-sum-lite"] = "assemble<2,->"
ISO_PRODUCT = dict(p=2, lengthscales=(0.9, 0.6, 1.3), v=(0.7, -0.4, 0.3), w=(-0.5, 0.9, 0.6), c=1.5, scale=1.3)
# (id, descriptor or "iso", asm_factors): one per kernel variant; (n0, n1) = (130, 150), set (a); 1, 4, 5 and 9 right-hand sides
PRODUCT_SMALL = [("matvec_fast<2,3,3,0>", "s2-q33-odd", 0), ("matvec_fast<2,3,5,1>", "s2-35-odd", 0), ("matvec_fast<2,5,3,2>", "s2-53-lap", 0),
                 ("matvec<2,->-sum", "g2-sum", 0), ("matvec<3,->", "g3", 0), ("matvec<3,->-iso", "iso", 0), ("matvec<2,F>", "s2-35-odd", 1)]
PRODUCT_SHAPE = (130, 150)
PRODUCT_RHS = (1, 4, 5, 9)
# the accumulation over several column tiles per split and the split without a tile: (name, row tiles as a function of the CU count,
# n1, the plan expected: splits, per, tiles per split)
PRODUCT_BIG = [("per2-empty-split", lambda cus: 64 * cus + 37, 300, (4, 2, [2, 2, 1, 0])),
               ("per2-splits2", lambda cus: 128 * cus - 27, 190, (2, 2, [2, 1]))]
PRODUCT_BIG_DESCRIPTORS = ("s2-35-odd", "g2-sum-lite")
BIG_ROWS = 96


def small_product_block(desc):
    """(X0, X1, Block) of a small product case (cached by the caller)."""
    n0, n1 = PRODUCT_SHAPE
    if desc == "iso":
        q = ISO_PRODUCT
        rng = np.random.default_rng(20241020)
        X0, X1 = rng.uniform(0.0, 3.0, (n0, 3)), rng.uniform(0.0, 3.0, (n1, 3))
        L0, L1 = iso_first_pairs(3, q["v"], q["w"], q["c"])["grad_grad"]
        return X0, X1, iso_first_block(q["p"], q["lengthscales"], L0, L1, X0, X1, q["scale"])
    kernel, L0, L1 = DESCRIPTORS[desc]
    X0, X1 = points(desc + "-product", kernel, len(next(iter(L0))), "off", n0, n1, "a")
    return X0, X1, scattered_block(kernel, L0, L1, X0, X1)


def big_rows(n0, seed):
    """About 96 rows of an n0-row product: the first row tile's edges, the last ragged tile, the rows at 64-row borders, random ones."""
    rng = np.random.default_rng(seed)
    last = 64 * ((n0 - 1) // 64)
    rows = {0, 1, 62, 63, 64, 65, 127, 128, n0 - 1, n0 - 2, last, last - 1, last + 1} | set(range(last, n0, 5))
    rows |= {int(64 * t + o) for t in rng.integers(1, (n0 - 1) // 64, 12) for o in (-1, 0)}
    rows = {r for r in rows if 0 <= r < n0}
    while len(rows) < BIG_ROWS:
        rows.add(int(rng.integers(0, n0)))
    return np.array(sorted(rows))


def big_product(name, desc, cus=256):
    """(X0, X1, V, rows, Block on the sampled rows) of a large product case."""
    _, n0_of, n1, _ = next(c for c in PRODUCT_BIG if c[0] == name)
    n0 = n0_of(cus)
    kernel, L0, L1 = DESCRIPTORS[desc]
    seed = sum(map(ord, name + desc))
    rng = np.random.default_rng(seed)
    X0, X1 = rng.uniform(0.0, 3.0, (n0, 2)), rng.uniform(0.0, 3.0, (n1, 2))
    V = rng.standard_normal((n1, 5))
    rows = big_rows(n0, seed)
    parts = [scattered_block(kernel, L0, L1, X0[rows[i:i + 48]], X1) for i in range(0, len(rows), 48)]
    cat = lambda f: np.concatenate([getattr(b, f) for b in parts])       # noqa: E731
    return X0, X1, V, rows, Block(*(cat(f) for f in ("G", "E", "W", "eta", "rho", "expo", "expo0")))
