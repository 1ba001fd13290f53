"""Long-double reference of leave-fold-out cross-validation computed from a GIVEN lower-triangular factor L (float64 in,
`np.longdouble` inside), in the pattern of _factor_reference.py: with L shared between the device and the reference the cond-bound
error of the factorisation drops out and a measure sees csrc/evidence_cv.hip alone (test_gpu_cv.py).  The formulas are those of
GPML section 5.4.2 (the block form of eqs. 5.10 - 5.12), with P = G^{-1} = L^{-T} L^{-1}, w = P r and, per fold B, S = P[B, B]:

    mean_B = y_B - S^{-1} w_B,   Sigma_B = S^{-1},   log p(y_B | y_-B) = -1/2 w_B^T S^{-1} w_B + 1/2 log det S - |B|/2 log 2 pi

`evaluate_float64` is the same evaluation in float64 on NumPy / SciPy (LAPACK): its distance from the long-double one is the
yardstick the device is held to.  Held to the definition -- delete the fold, condition on the rest, predict the fold -- in
test_cv_reference.py.  A plain module the suites import, not a conftest."""
import numpy as np
import scipy.linalg

import _factor_reference as fr

LD = fr.LD
HALF_LOG_2PI = fr.HALF_LOG_2PI


def cholesky_ld(A):
    """Lower Cholesky factor of a symmetric positive definite long-double matrix, by rows."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    C = np.zeros((n, n), dtype=LD)
    for i in range(n):
        for j in range(i):
            C[i, j] = (A[i, j] - C[i, :j] @ C[j, :j]) / C[j, j]
        d = A[i, i] - C[i, :i] @ C[i, :i]
        assert d > 0, f"pivot {i} is not positive"
        C[i, i] = np.sqrt(d)
    return C


def solve_spd_ld(C, B):
    """(C C^T)^{-1} B for a lower long-double factor C; B a vector or a matrix."""
    B = np.asarray(B, dtype=LD)
    n = C.shape[0]
    Z = np.zeros_like(B)
    for i in range(n):
        Z[i] = (B[i] - C[i, :i] @ Z[:i]) / C[i, i]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (Z[i] - C[i + 1:, i] @ X[i + 1:]) / C[i, i]
    return X


class CvResult:
    """mean, var: (n,), NaN outside the folds; logp: (nfolds,); total; cov: list of (b, b)."""

    def __init__(self, mean, var, logp, total, cov):
        self.mean, self.var, self.logp, self.total, self.cov = mean, var, logp, total, cov


def inverse_and_weights(L, r):
    """P = L^{-T} L^{-1} and w = P r in long double."""
    W = fr.inverse(L)
    P = W.T @ W
    return P, W.T @ (W @ np.asarray(r).astype(LD))


def evaluate(L, r, y, folds):
    """The formulas at the top in long double from the factor L; `folds`: index arrays, rows of a fold in increasing order."""
    n = L.shape[0]
    P, w = inverse_and_weights(L, r)
    yl = np.asarray(y).astype(LD)
    mean, var = np.full(n, np.nan, dtype=LD), np.full(n, np.nan, dtype=LD)
    logp, covs = np.zeros(len(folds), dtype=LD), []
    for f, B in enumerate(folds):
        B = np.asarray(B)
        C = cholesky_ld(P[np.ix_(B, B)])
        x = solve_spd_ld(C, w[B])
        Sigma = solve_spd_ld(C, np.eye(B.size, dtype=LD))
        mean[B] = yl[B] - x
        var[B] = np.diag(Sigma)
        logp[f] = -LD(0.5) * (w[B] @ x) + np.sum(np.log(np.diag(C))) - B.size * HALF_LOG_2PI
        covs.append(Sigma)
    total = LD(0)
    for v in logp:                                # fold order
        total = total + v
    return CvResult(mean, var, logp, total, covs)


def evaluate_float64(L, r, y, folds):
    """The same formulas in float64 with LAPACK (scipy.linalg): the second, equally valid double evaluation whose distance from
    `evaluate` is the yardstick of test_gpu_cv.py."""
    n = L.shape[0]
    W = scipy.linalg.solve_triangular(L, np.eye(n), lower=True)
    P = W.T @ W
    w = scipy.linalg.cho_solve((L, True), np.asarray(r, dtype=np.float64))
    mean, var = np.full(n, np.nan), np.full(n, np.nan)
    logp, covs = np.zeros(len(folds)), []
    for f, B in enumerate(folds):
        B = np.asarray(B)
        C = scipy.linalg.cholesky(P[np.ix_(B, B)], lower=True)
        x = scipy.linalg.cho_solve((C, True), w[B])
        Sigma = scipy.linalg.cho_solve((C, True), np.eye(B.size))
        mean[B] = y[B] - x
        var[B] = np.diag(Sigma)
        logp[f] = -0.5 * (w[B] @ x) + np.sum(np.log(np.diag(C))) - B.size * float(HALF_LOG_2PI)
        covs.append(Sigma)
    return CvResult(mean, var, logp, float(np.sum(logp)), covs)


def by_definition(G, r, y, B):
    """Leave fold B out BY DEFINITION, in long double: delete its rows and columns from G, condition on the rest, predict the fold
    with its own noise (G carries it).  With R the other rows and the prior mean m = y - r:
        mean_B = m_B + G_BR G_RR^{-1} r_R,   Sigma_B = G_BB - G_BR G_RR^{-1} G_RB,   log p = log N(y_B; mean_B, Sigma_B).
    B = all rows: the marginal distribution N(m, G).  Returns (mean_B, Sigma_B, logp)."""
    Gl, rl, yl = np.asarray(G).astype(LD), np.asarray(r).astype(LD), np.asarray(y).astype(LD)
    B = np.asarray(B)
    R = np.setdiff1d(np.arange(Gl.shape[0]), B)
    m = yl - rl
    mean, Sigma = m[B].copy(), Gl[np.ix_(B, B)].copy()
    if R.size:
        C = cholesky_ld(Gl[np.ix_(R, R)])
        GRB = Gl[np.ix_(R, B)]
        mean = mean + GRB.T @ solve_spd_ld(C, rl[R])
        Sigma = Sigma - GRB.T @ solve_spd_ld(C, GRB)
    Cs = cholesky_ld(Sigma)
    e = yl[B] - mean
    logp = -LD(0.5) * (e @ solve_spd_ld(Cs, e)) - np.sum(np.log(np.diag(Cs))) - B.size * HALF_LOG_2PI
    return mean, Sigma, logp


def distance(got, ref):
    """max |got - ref| over the entries where ref is finite, relative to max |ref| there (the measure of the yardstick); where ref is
    NaN, got must be NaN too."""
    got, ref = np.asarray(got).astype(LD), np.asarray(ref).astype(LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.all(np.isnan(got[~fin])), "a value where the reference has none"
    assert np.all(np.isfinite(got[fin])), "a NaN or an infinity where the reference has a value"
    return float(np.max(np.abs(got[fin] - ref[fin])) / np.max(np.abs(ref[fin])))


class Problem220:
    """The problem of test_gpu_cv.py, stated once: prior GP(0, Matern-5/2, lengthscale 0.5) on [-1, 1]; 150 noisy values at scattered
    points, then 70 noisy first derivatives at other points, noise variance 1e-2 each.  n = 220, 256 + 128 = 384 padded rows: the
    map from Gram rows to padded rows has a gap in the middle."""
    kernel = [(1.0, [("matern", 2.5, 0.5)])]
    sizes = (150, 70)
    noise = 1e-2

    def __init__(self):
        rng = np.random.default_rng(220)
        self.X = [rng.uniform(-1.0, 1.0, (150, 1)), rng.uniform(-1.0, 1.0, (70, 1))]
        self.ops = [{(0,): 1.0}, {(1,): 1.0}]
        self.Y = [np.sin(3.0 * self.X[0][:, 0]) + 0.1 * rng.standard_normal(150), 3.0 * np.cos(3.0 * self.X[1][:, 0]) + 0.1 * rng.standard_normal(70)]
        self.n = 220
        self.y = np.concatenate(self.Y)

    def oracle_blocks(self):
        from oracle import gp as ogp
        return [ogp.ObsBlock(X, op, Y, None, self.noise) for X, op, Y in zip(self.X, self.ops, self.Y)]

    def gram(self):
        from oracle import gp as ogp
        return ogp.gram(self.kernel, self.oracle_blocks())

    @staticmethod
    def mixed_folds():
        """A fixed permutation of the 220 rows cut into folds of 1, 2, 16, 17, 127 and 57 rows (sorted); every fold of more than one
        row has rows of both observation blocks."""
        for seed in range(100):
            perm = np.random.default_rng(seed).permutation(220)
            cuts = np.cumsum([0, 1, 2, 16, 17, 127, 57])
            folds = [np.sort(perm[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
            if all(f.min() < 150 <= f.max() for f in folds[1:]):
                return folds
        raise AssertionError("no permutation found")

    @staticmethod
    def boundary_folds():
        """Two fold sets on the two sides of the 128-row threshold, the remaining rows in no fold: [128 rows], and [129 rows, 50 rows]
        (128 + 129 rows do not fit into 220 disjointly: two calls)."""
        perm = np.random.default_rng(128).permutation(220)
        return [np.sort(perm[:128])], [np.sort(perm[:129]), np.sort(perm[129:179])]
