"""tests/_factor_reference.py (the long-double references of test_gpu_evidence_backward.py and test_gpu_solve_t_backward.py)
against 50-digit mpmath at n = 40, and LAPACK's own distance from those references on the matrices the GPU suite uses.  No GPU.

The references must be good to a small fraction of one u = 2^-53 on the cases where a double result is a few u off, or a
measure "in units of u" means nothing: against mpmath every reference is held to REF_TOL = u / 64 in the measure the GPU suite
takes of it -- z by its componentwise backward error, a column of L^-1 relative to its 2-norm, d, the logs and the LOO formulas
componentwise (long double carries 11 more bits; the cases are a factor whose diagonal straddles 1, so that the logs change
sign, and one whose rows are scaled over twelve decades).  The GPU suite states its bars as multiples of LAPACK's error on the same factor; a LAPACK
error that is large would make such a bar vacuous, so LAPACK is held here to caps taken from its own measured error on NumPy
factors of the same matrices (Matern-5/2, lengthscale 0.3, scattered 2-D points, the three noise kinds of _backward.py):
  z = L^-1 r       componentwise backward error of scipy.linalg.solve_triangular   <= CAP_Z = 8 u     [measured: 0.6 - 5.2 u]
  d = diag(G^-1)   componentwise relative error of solve_triangular(L, I), column sums of squares in double
                                                                                    <= CAP_D = 256 u   [measured: 3.7 - 163 u]
  2 sum log L_ii   |numpy's double value - reference| <= CAP_LOG = 32 u 2 sum |log L_ii| (the ceiling of the device's bar)  [measured: at most 1.24 u]"""
import mpmath
import numpy as np
import pytest
import scipy.linalg

import _factor_reference as fr
from _backward import gram_points

U = fr.U
LD = fr.LD
REF_TOL = U / 64
CAP_Z, CAP_D, CAP_LOG = 8 * U, 256 * U, 32 * U
DPS = 50


def matern52_gram(kind, n):
    X, noise = gram_points(kind, n)
    r = np.sqrt(5.0) * np.sqrt(np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=-1)) / 0.3
    return (1 + r + r * r / 3) * np.exp(-r) + np.diag(noise)


def small_factor(case):
    """n = 40 lower-triangular factors: "straddle": the Cholesky factor of a Matern Gram scaled so that its diagonal runs over
    [0.03, 30] on both sides of 1; "decades": rows scaled over twelve decades."""
    rng = np.random.default_rng(40 + len(case))
    L = np.linalg.cholesky(matern52_gram("m", 40))
    s = 10.0 ** rng.uniform(-1.5, 1.5, 40) if case == "straddle" else 10.0 ** rng.uniform(-6, 6, 40)
    L = s[:, None] * L
    return L, rng.standard_normal(40) * (s if case == "decades" else 1.0), rng.standard_normal(40)


def mp_forward(L, r):
    n = L.shape[0]
    z = [mpmath.mpf(0)] * n
    for i in range(n):
        z[i] = (mpmath.mpf(float(r[i])) - mpmath.fsum(mpmath.mpf(float(L[i, j])) * z[j] for j in range(i))) / mpmath.mpf(float(L[i, i]))
    return z


def mp_inverse(L):
    n = L.shape[0]
    Lm = [[mpmath.mpf(float(L[i, j])) for j in range(n)] for i in range(n)]
    W = [[mpmath.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for c in range(i + 1):
            W[i][c] = ((1 if c == i else 0) - mpmath.fsum(Lm[i][j] * W[j][c] for j in range(c, i))) / Lm[i][i]
    return W


def as_mp(x):
    """A long double as an exact mpmath number (hi + lo split: mpf() of a numpy long double goes through float)."""
    hi = np.float64(x)
    lo = np.float64(x - LD(hi))
    return mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))


def rel_ld(got, want):
    worst = mpmath.mpf(0)
    for g, w in zip(np.asarray(got, dtype=LD).reshape(-1), want):
        gm = as_mp(g)
        worst = max(worst, abs(gm - w) / abs(w) if w != 0 else abs(gm))
    return float(worst)


@pytest.mark.parametrize("case", ["straddle", "decades"])
def test_references_against_mpmath(case):
    L, r, y = small_factor(case)
    diag = np.diag(L)
    if case == "straddle":
        assert diag.min() < 0.5 and diag.max() > 2.0
    else:
        assert np.ptp(np.log10(np.abs(L).max(axis=1))) >= 10.0
    with mpmath.workdps(DPS):
        z = mp_forward(L, r)
        # an entry of z is a sum that may cancel (rows over twelve decades: its relative error is cond-bound in any
        # precision); what the reference owes is a componentwise backward error far below u -- and backward_error() itself
        # must agree with the same measure taken in mpmath
        zl = fr.forward(L, r)
        print(f"\n[{case}] forward: relative error {rel_ld(zl, z) / U:.2e} u")
        Lm = [[mpmath.mpf(float(L[i, j])) for j in range(i + 1)] for i in range(40)]
        zm = [as_mp(v) for v in zl]
        e = max(float(abs(mpmath.mpf(float(r[i])) - mpmath.fsum(Lm[i][j] * zm[j] for j in range(i + 1)))
                      / (mpmath.fsum(abs(Lm[i][j] * zm[j]) for j in range(i + 1)) + abs(mpmath.mpf(float(r[i]))))) for i in range(40))
        print(f"[{case}] forward: componentwise backward error {e / U:.2e} u")
        assert e <= REF_TOL
        zd = zl.astype(np.float64)                 # rounded to double the residual is large enough for long double to measure
        zdm = [mpmath.mpf(float(v)) for v in zd]
        want = max(float(abs(mpmath.mpf(float(r[i])) - mpmath.fsum(Lm[i][j] * zdm[j] for j in range(i + 1)))
                         / (mpmath.fsum(abs(Lm[i][j] * zdm[j]) for j in range(i + 1)) + abs(mpmath.mpf(float(r[i]))))) for i in range(40))
        assert abs(fr.backward_error(L, zd, r) - want) <= REF_TOL and want <= 2 * U
        W = mp_inverse(L)
        Wl = fr.inverse(L)
        assert np.all(np.triu(Wl, 1) == 0)
        # an entry of L^-1 is a sum that may cancel: no precision gives it to a relative error.  What d = colsum(W * W) needs
        # is every column to a fraction of its own 2-norm
        e = max(float(mpmath.sqrt(mpmath.fsum((as_mp(Wl[i, j]) - W[i][j]) ** 2 for i in range(j, 40)) / mpmath.fsum(W[i][j] ** 2 for i in range(j, 40))))
                for j in range(40))
        print(f"[{case}] inverse: {e / U:.2e} u of a column's norm")
        assert e <= REF_TOL
        d = [mpmath.fsum(W[i][j] ** 2 for i in range(j, 40)) for j in range(40)]
        dl = fr.inverse_diag(Wl)
        e = rel_ld(dl, d)
        print(f"[{case}] inverse diagonal: {e / U:.2e} u; d spans {float(min(d)):.1e} .. {float(max(d)):.1e}")
        assert e <= REF_TOL
        logs = [mpmath.log(mpmath.mpf(float(v))) for v in diag]
        ld, scale = fr.logdet(diag)
        e = float(abs(as_mp(ld) - 2 * mpmath.fsum(logs)) / (2 * mpmath.fsum(abs(v) for v in logs)))
        print(f"[{case}] log det: {e / U:.2e} u of 2 sum |log|; log det {float(ld):.3f}, 2 sum |log| {float(scale):.3f}")
        assert e <= REF_TOL
        assert float(abs(as_mp(scale) - 2 * mpmath.fsum(abs(v) for v in logs))) <= REF_TOL * float(scale)
        if case == "straddle":
            assert abs(float(ld)) < 0.5 * float(scale)          # the logs cancel: the scale is not |log det|
        # the LOO formulas from (w, d, y), w any vector
        w = np.random.default_rng(3).standard_normal(40) * np.sqrt(np.asarray(dl, dtype=np.float64))
        dd = np.asarray(dl, dtype=np.float64)
        mean, var, logp = fr.loo(w, dd, y)
        wm, dm, ym = ([mpmath.mpf(float(v)) for v in a] for a in (w, dd, y))
        e = max(rel_ld(var, [1 / v for v in dm]),
                rel_ld(logp, [mpmath.log(v) / 2 - a * a / v / 2 - mpmath.log(2 * mpmath.pi) / 2 for a, v in zip(wm, dm)]))
        print(f"[{case}] LOO var, logp: {e / U:.2e} u")
        assert e <= REF_TOL
        # the mean cancels (y - w / d): its error is stated against |y| + |w / d|
        mm = [b - a / v for a, v, b in zip(wm, dm, ym)]
        e = max(float(abs(as_mp(g) - m) / (abs(b) + abs(a / v))) for g, m, a, v, b in zip(mean, mm, wm, dm, ym))
        assert e <= REF_TOL


def test_backward_error_conventions():
    L = np.array([[2.0, 0.0, 0.0], [1.0, 4.0, 0.0], [0.0, 0.0, 1.0]])
    z = np.array([1.0, 0.5, 0.0])
    r = L @ z
    assert fr.backward_error(L, z, r) == 0.0                              # the last row: 0 / 0 counts 0
    r2 = r.copy()
    r2[1] += 3.0 * 2.0 ** -50                                              # (r_1 = 3: |L||z| + |r| = 6 + a rounding)
    assert abs(fr.backward_error(L, z, r2) - 3.0 * 2.0 ** -50 / 6.0) <= 1e-28
    zbad = z.copy()
    zbad[2] = 1e-300                                                       # a nonzero over a nonzero denominator: a number
    assert fr.backward_error(L, zbad, r) == 1.0
    Lz = np.array([[1.0, 0.0], [1.0, 0.0]])                                # |L||z| + |r| = 0 in both rows, r - L z = 0
    assert fr.backward_error(Lz, np.array([0.0, 5.0]), np.zeros(2)) == 0.0
    assert np.isnan(fr.backward_error(L, np.array([1.0, np.nan, 0.0]), r))   # a NaN stays a NaN: no bar is met by it
    assert fr.relative_error(np.array([1.0 + 2.0 ** -52, 0.0]), np.array([1.0, 0.0])) == 2.0 ** -52
    with pytest.raises(AssertionError, match="exactly zero"):
        fr.relative_error(np.array([1e-300]), np.array([0.0]))


_lapack = {}


def lapack_case(kind, n):
    if (kind, n) not in _lapack:
        G = matern52_gram(kind, n)
        L = np.linalg.cholesky(G)
        _lapack[(kind, n)] = (L, fr.inverse_diag(fr.inverse(L)))
    return _lapack[(kind, n)]


@pytest.mark.parametrize("n", [100, 128, 300, 700])
@pytest.mark.parametrize("kind", ["m", "b", "s"])
def test_lapack_stays_within_the_caps(kind, n):
    """LAPACK on a NumPy factor of the GPU suite's matrices: the denominators of RATIO_Z and RATIO_D are a few u, not a bar
    that anything passes."""
    L, d_ref = lapack_case(kind, n)
    r = np.random.default_rng(n + 1).standard_normal(n)
    be = fr.backward_error(L, scipy.linalg.solve_triangular(L, r, lower=True), r)
    ref = fr.forward(L, r)
    assert fr.backward_error(L, ref.astype(np.float64), r) <= 2 * U          # the rounded reference: one rounding per entry
    W = scipy.linalg.solve_triangular(L, np.eye(n), lower=True)
    ed = fr.relative_error(np.sum(W * W, axis=0), d_ref)
    diag = np.diag(L)
    ld, scale = fr.logdet(diag)
    el = float(abs(LD(2.0 * np.sum(np.log(diag))) - ld) / scale)
    span = float(np.log10(float(d_ref.max()) / float(d_ref.min())))
    print(f"\n[{kind} n={n}] solve_triangular backward error {be / U:.2f} u; diag(G^-1) relative error {ed / U:.1f} u over {span:.1f} decades; "
          f"log det {el / U:.2f} u of 2 sum |log| ({float(ld):.1f} of {float(scale):.1f})")
    assert be <= CAP_Z
    assert ed <= CAP_D
    assert el <= CAP_LOG
    if kind == "s":
        assert span >= 8.0


# ---- the transposed product and its backward error (test_gpu_solve_t_backward.py) ------------------------------------------
def mp_backward_error_t(L, x, y):
    """max_i |y - L^T x|_i / (|L^T||x| + |y|)_i in mpmath; x, y doubles or long doubles."""
    n = L.shape[0]
    xm, ym = [as_mp(v) for v in x], [as_mp(v) for v in y]
    worst = mpmath.mpf(0)
    for i in range(n):
        col = [mpmath.mpf(float(L[j, i])) * xm[j] for j in range(i, n)]
        den = mpmath.fsum(abs(v) for v in col) + abs(ym[i])
        res = abs(ym[i] - mpmath.fsum(col))
        assert den != 0 or res == 0
        if den != 0:
            worst = max(worst, res / den)
    return float(worst)


@pytest.mark.parametrize("case", ["straddle", "decades"])
def test_transposed_references_against_mpmath(case):
    L, r, y = small_factor(case)
    with mpmath.workdps(DPS):
        # L^T x itself, relative to |L|^T |x| (a sum that may cancel has no relative error in any precision)
        got, scale = fr.lower_tmv(L, r), fr.lower_tmv(L, r, absolute=True)
        want = [mpmath.fsum(mpmath.mpf(float(L[j, i])) * mpmath.mpf(float(r[j])) for j in range(i, 40)) for i in range(40)]
        wabs = [mpmath.fsum(abs(mpmath.mpf(float(L[j, i])) * mpmath.mpf(float(r[j]))) for j in range(i, 40)) for i in range(40)]
        e = max(float(abs(as_mp(g) - w) / a) for g, w, a in zip(got, want, wabs))
        print(f"\n[{case}] L^T x: {e / U:.2e} u of |L|^T |x|")
        assert e <= REF_TOL and rel_ld(scale, wabs) <= REF_TOL
        # backward_error_t of LAPACK's double solution: the same measure in mpmath
        for rhs in (r, y):
            xd = scipy.linalg.solve_triangular(L, rhs, lower=True, trans="T")
            be, want = fr.backward_error_t(L, xd, rhs), mp_backward_error_t(L, xd, rhs)
            print(f"[{case}] backward error of solve_triangular(trans='T') {be / U:.3f} u (mpmath {want / U:.3f} u)")
            assert abs(be - want) <= REF_TOL and 0 < want <= CAP_Z
        # columns of a matrix are measured one by one
        X = np.stack([scipy.linalg.solve_triangular(L, v, lower=True, trans="T") for v in (r, y)], axis=1)
        per_col = fr.backward_error_t(L, X, np.stack([r, y], axis=1))
        assert per_col.shape == (2,) and per_col[0] == fr.backward_error_t(L, X[:, 0], r) and per_col[1] == fr.backward_error_t(L, X[:, 1], y)


def test_transposed_product_across_row_slabs():
    """Above 512 rows lower_tmv() adds the slabs' contributions up: at n = 600 (slabs of 512 and 88 rows) against mpmath on the
    columns a slab boundary cuts, at the a-priori bound of a long-double sum of n terms, n 2^-64 of |L|^T |x| (= 0.29 u at
    n = 600: what a measure "in u" of the GPU suite can be off by at that size; the error measured here is far smaller)."""
    n = 600
    L = np.linalg.cholesky(matern52_gram("b", n))
    x = np.random.default_rng(n).standard_normal(n)
    got, scale = fr.lower_tmv(L, x), fr.lower_tmv(L, x, absolute=True)
    with mpmath.workdps(DPS):
        worst = 0.0
        for i in (0, 1, 255, 510, 511, 512, 513, 598, 599):
            want = mpmath.fsum(mpmath.mpf(float(L[j, i])) * mpmath.mpf(float(x[j])) for j in range(i, n))
            worst = max(worst, float(abs(as_mp(got[i]) - want) / as_mp(scale[i])))
    print(f"\nL^T x at n = {n}: {worst / U:.2e} u of |L|^T |x|")
    assert worst <= n * 2.0 ** -64
    assert np.all(np.triu(L, 1) == 0)


def test_backward_error_t_conventions():
    L = np.array([[2.0, 0.0, 0.0], [1.0, 4.0, 0.0], [0.0, 0.0, 1.0]])
    x = np.array([1.0, 0.5, 0.0])
    y = L.T @ x
    assert fr.backward_error_t(L, x, y) == 0.0                             # the last row: 0 / 0 counts 0
    y2 = y.copy()
    y2[0] += 2.5 * 2.0 ** -50                                              # (y_0 = 2.5: |L^T||x| + |y| = 5 + a rounding)
    assert abs(fr.backward_error_t(L, x, y2) - 2.5 * 2.0 ** -50 / 5.0) <= 1e-28
    Lz = np.array([[0.0, 0.0], [0.0, 1.0]])                                # column 0 of L is zero: |L^T||x| + |y| = 0 in row 0
    assert fr.backward_error_t(Lz, np.array([5.0, 0.0]), np.zeros(2)) == 0.0
    xbad = x.copy()
    xbad[2] = 1e-300                                                       # a nonzero over a nonzero denominator: a number
    assert fr.backward_error_t(L, xbad, y) == 1.0
    assert np.isnan(fr.backward_error_t(L, np.array([1.0, np.nan, 0.0]), y))  # a NaN stays a NaN: no bar is met by it


# ---- the depth-aware bounds of the two-stage reductions (test_gpu_evidence_backward.py, capped launches) -----------------------
def test_reduction_depth_by_hand():
    """k = ceil(pn / (256 nwg)), nwg = min(ceil(pn / 256), 256, cap): the cases of the GPU suite and the edges of the uncapped launch."""
    assert fr.reduction_workgroups(768) == 3 and fr.reduction_workgroups(768, 1) == 1 and fr.reduction_workgroups(768, 2) == 2
    assert fr.reduction_workgroups(768, 5) == 3                       # a cap above what the size asks for changes nothing
    assert (fr.reduction_depth(768), fr.reduction_depth(768, 2), fr.reduction_depth(768, 1)) == (1, 2, 3)
    assert (fr.reduction_depth(128), fr.reduction_depth(384, 1), fr.reduction_depth(512, 1)) == (1, 2, 2)
    assert fr.reduction_workgroups(65536) == 256 and fr.reduction_depth(65536) == 1        # 256 x 256: the last size of one row per thread
    assert fr.reduction_workgroups(65664) == 256 and fr.reduction_depth(65664) == 2        # one tile row more: the stride loop repeats


def test_bounds_at_depth_1_2_3_by_hand():
    """17, 18, 19 roundings; at k = 1 the constants the uncapped tests have always used (SUM_ULPS = 20, LOG_ULPS = 7)."""
    assert [fr.sum_roundings(k) for k in (1, 2, 3)] == [17, 18, 19]
    assert [fr.sum_ulps(k) for k in (1, 2, 3)] == [20.0, 21.0, 22.0]
    assert [fr.log_ulps(k) for k in (1, 2, 3)] == [7.0, 8.0, 9.0]
    for k in (1, 2, 3, 64):
        m = fr.sum_roundings(k)
        assert float((LD(1) + LD(U)) ** m - 1) < fr.sum_ulps(k) * U       # what the bound claims of m roundings


@pytest.mark.parametrize("pn,cap", [(768, 0), (768, 2), (768, 1), (384, 1), (1408, 1)])
def test_host_model_of_the_reduction_meets_the_bound(pn, cap):
    """`two_stage_sum`, the host model of the order of summation, on non-negative terms over twelve decades: exact on integers
    (nothing lost, nothing twice), and within sum_ulps(k) u of the long-double sum otherwise (the bound of a sum in ANY order, one
    rounding per term, would be pn u)."""
    rng = np.random.default_rng(pn + cap)
    nwg, k = fr.reduction_workgroups(pn, cap), fr.reduction_depth(pn, cap)
    ints = rng.integers(0, 65, pn).astype(np.float64)
    assert fr.two_stage_sum(ints, nwg) == float(np.sum(ints.astype(np.int64)))
    worst = 0.0
    for _ in range(20):
        terms = rng.uniform(0, 1, pn) * 10.0 ** rng.uniform(-6, 6, pn)
        ref = np.sum(terms.astype(LD))
        worst = max(worst, float(abs(LD(fr.two_stage_sum(terms, nwg)) - ref) / (U * ref)))
    print(f"two-stage sum pn={pn} cap={cap}: k={k}, worst error {worst:.2f} u of the sum, bound {fr.sum_ulps(k):.0f} u")
    assert worst <= fr.sum_ulps(k) < pn
