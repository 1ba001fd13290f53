"""Dense high-precision reference of the matrix-free SOLVE (`randprocs/_matrix_free.py`: `PivotedCholeskyPreconditioner`, `pcg`,
`pcg_device`, `_solve`) and the cases of the suites (test_mfree_reference.py on the CPU, test_gpu_mfree_solve.py on the device).
A plain module, not a conftest: NumPy and the oracle, no device code.

* `DenseGram(A)`: the part of `GramProduct` the preconditioner and `pcg` use, on a dense float64 matrix; it records the rows it
  was asked for, which are the pivots of the pivoted Cholesky in their order.
* `case(kernel, n, noise)`: points uniform in [-1, 1]^2, the oracle's Gram matrix G (`oracle.gp.condition(...).G`), standard
  normal right-hand sides, kappa_2(G) by `numpy.linalg.cond` and the rtol the case runs at.  `prior(lp, kernel)` and
  `observe(lp, prior, case)` put the same points through the package.
* `reference_cg`: the iteration of `pcg` in `np.longdouble`, preconditioned by `ReferencePreconditioner`: M = L^T L + delta I with
  the class's own L and delta, applied by a dense solve (float64 inverse of M, refined on longdouble residuals down to the
  rounding of the residual itself).  What it applies is M^-1, not a Woodbury form of it.
* `DeviceFormPreconditioner`: the float64 form `pcg_device` hands to the device, Z = (R - L^T (Sinv (L R))) / delta with Sinv the
  symmetrised explicit inverse of the small matrix.
* `true_residual(G, X, B)`: ||B - G X|| / ||B|| per column in longdouble.

The case rule.  A case runs at rtol = 1e-10 if u kappa_2(G) <= 1e-11, otherwise at 1e-6 (u = 2^-53): the recurrence residual CG
stops on and the true residual part by about u kappa_2(G), so under the rule (u kappa_2 <= rtol / 10, asserted on the CPU for
every case) rounding explains a true residual of 1.1 rtol and anything beyond 2 rtol is drift.  A condition on the inputs, not a
measurement.

The slack.  `pcg` (host form and device form) may take `slack(it_ref)` iterations beyond the reference's count it_ref:
  SLACK = 2 where it_ref <= SHORT = 16: float64 rounding near the stopping threshold delays the last step; the worst excess measured over the
      grid where the reference takes at most 16 iterations is +1, and SLACK is twice that;
  DELAY * it_ref beyond: conjugate gradients in finite precision lose the orthogonality of their directions and fall behind
      the exact recurrence in proportion to the iterations taken (Greenbaum 1989) -- a property of float64, not of this code.  The
      worst measured excess is 57 % of the reference's count (plain CG, ExpQuad, n = 333, noise 1e-6: 1 483 against 944; 20 to
      31 % at rank 17); DELAY is twice that.
One number for the whole grid, twice the worst excess (+539), would pass a solve that takes 6 iterations where the reference takes 1:
the defect the suite is there to catch.  `slack` is nowhere wider than that number and tight where the solves are short
(MEASUREMENTS.md, "Matrix-free solves against a dense reference")."""
import dataclasses
import functools

import numpy as np

from oracle import covfuncs as ocf
from oracle import gp as ogp

import _pcg_reference as pr

LD, U = pr.LD, pr.U

LENGTHSCALE = 0.7
KERNELS = {
    "matern52": [(1.0, [("matern", 2.5, LENGTHSCALE), ("matern", 2.5, LENGTHSCALE)])],
    "expquad": [(1.0, [("expquad", LENGTHSCALE), ("expquad", LENGTHSCALE)])],
}
SIZES = (1, 3, 64, 150, 200, 201, 333)
NOISES = (1e-2, 1e-6)
RANKS = (200, 0, 17)          # 200 is `config.matrix_free_preconditioner_rank`'s default
COLUMNS = 3
DELTA_FLOOR = 1e-8            # the documented rule: delta = max(mean of the unexplained diagonal, DELTA_FLOOR * max diag G)
PIVOT_RTOL = 1e-6             # the class's default `rtol`: pivoting stops at a remaining diagonal <= PIVOT_RTOL * max diag G
SLACK = 2
DELAY = 1.14
SHORT = 16                    # iterations up to which a solve counts as short


def slack(it_ref):
    return SLACK if it_ref <= SHORT else max(SLACK, int(np.ceil(DELAY * it_ref)))


class DenseGram:
    """`n`, `diag()`, `row(p)`, `matvec` of `GramProduct` on a dense matrix."""

    def __init__(self, A):
        self.A = np.array(A, dtype=np.double)
        self.n = self.A.shape[0]
        self.rows_asked = []

    @property
    def shape(self):
        return self.A.shape

    def diag(self):
        return np.diag(self.A).copy()

    def row(self, p):
        self.rows_asked.append(int(p))
        return self.A[int(p)].copy()

    def matvec(self, V):
        return self.A @ np.asarray(V, dtype=np.double)

    __matmul__ = matvec


def rtol_for(kappa):
    return 1e-10 if U * kappa <= 1e-11 else 1e-6


@dataclasses.dataclass(frozen=True)
class Case:
    kernel: str
    n: int
    noise: float
    X: np.ndarray
    G: np.ndarray
    B: np.ndarray
    kappa: float
    rtol: float

    def __repr__(self):
        return f"{self.kernel} n={self.n} noise={self.noise:g}"


@functools.lru_cache(maxsize=None)
def case(kernel, n, noise, columns=COLUMNS):
    """The points depend on n alone (every kernel and noise level sees the same ones), the right-hand sides on n and `columns`."""
    X = np.random.default_rng([17, n]).uniform(-1.0, 1.0, (n, 2))
    B = np.random.default_rng([18, n, columns]).standard_normal((n, columns))
    G = ogp.condition(KERNELS[kernel], [ogp.ObsBlock(X, ocf.identity(2), B[:, 0], 0.0, noise)]).G
    kappa = float(np.linalg.cond(G))
    for a in (X, G, B):
        a.setflags(write=False)
    return Case(kernel, n, noise, X, G, B, kappa, rtol_for(kappa))


def prior(lp, kernel):
    cf = lp.randprocs.covfuncs
    one = {"matern52": lambda: cf.Matern((), nu=2.5, lengthscales=LENGTHSCALE), "expquad": lambda: cf.ExpQuad((), lengthscales=LENGTHSCALE)}[kernel]
    return lp.GaussianProcess(lp.functions.Zero((2,)), cf.TensorProduct(one(), one()))


def observe(lp, gp, c):
    """The case's points as one value block with a noise VECTOR (a diagonal: the device-resident loop applies)."""
    return gp.condition_on_observations(np.array(c.B[:, 0]), np.array(c.X), b=lp.randvars.Normal(np.zeros(c.n), np.full(c.n, c.noise)))


# ---- preconditioners ------------------------------------------------------------------------------------------------------------
class ReferencePreconditioner:
    """Z = M^-1 R, M = L^T L + delta I, as accurately as longdouble carries it: Z0 = inv(M) R in float64, then Z += inv(M) (R - M Z)
    with the residual in longdouble (M applied as L^T (L Z) + delta Z, never formed) until the residual is down at the rounding of
    its own evaluation, 2 (rank + 2) 2^-64 (|L|^T |L| |Z| + delta |Z|) in norm.  That is kappa_2(M) 2^-64 of Z where the float64
    Woodbury form is kappa_2(M) 2^-53: 2^-11 of the error of what it stands in for.  The sweeps contract by ~ u kappa_2(M); a
    run that does not get there fails its assertion, it does not return."""

    def __init__(self, L, delta):
        self.L64 = np.asarray(L, dtype=np.double)
        self.rank, self.n = self.L64.shape
        self.L = self.L64.astype(LD)
        self.absL = np.abs(self.L64)
        self.delta = float(delta)
        assert self.delta > 0.0
        self.Minv = np.linalg.inv(self.L64.T @ self.L64 + self.delta * np.eye(self.n)) if self.rank else None
        self.sweeps = 0

    def mul(self, Z):
        Z = np.asarray(Z).astype(LD)
        return self.L.T @ (self.L @ Z) + LD(self.delta) * Z

    def solve(self, R):
        R = np.asarray(R).astype(LD)
        if self.rank == 0:
            return R / LD(self.delta)
        Z = (self.Minv @ R.astype(np.double)).astype(LD)
        for sweep in range(60):
            Res = (R - self.mul(Z)).astype(np.double)
            Za = np.abs(Z.astype(np.double))
            floor = 2.0 * (self.rank + 2) * 2.0 ** -64 * (self.absL.T @ (self.absL @ Za) + self.delta * Za)
            if np.all(np.linalg.norm(Res, axis=0) <= np.linalg.norm(floor, axis=0)):
                self.sweeps = max(self.sweeps, sweep)
                return Z
            Z = Z + (self.Minv @ Res).astype(LD)
        raise AssertionError(f"the refinement of M^-1 R did not contract (rank {self.rank}, delta {self.delta:.3e})")


class DeviceFormPreconditioner:
    """What `pcg_device` gives `lpgp_pcg_create`, evaluated in float64 NumPy: Z = (R - L^T (Sinv (L R))) / delta, Sinv the explicit
    inverse of the class's `_chol _chol^T`, symmetrised."""

    def __init__(self, pre):
        self.L, self.delta, self.rank = pre.L, pre.delta, pre.rank
        if pre.rank:
            Sinv = np.linalg.inv(pre._chol @ pre._chol.T)
            self.Sinv = 0.5 * (Sinv + Sinv.T)

    def solve(self, R):
        if not self.rank:
            return R / self.delta
        return (R - self.L.T @ (self.Sinv @ (self.L @ R))) / self.delta


def applied_residual(form, pre, R):
    """||M (form.solve(R)) - R|| / ||R|| per column, M = L^T L + delta I in longdouble: is the preconditioner that is applied the
    one that was built?"""
    ref = ReferencePreconditioner(pre.L, pre.delta)
    D = ref.mul(form.solve(np.asarray(R, dtype=np.double))) - np.asarray(R).astype(LD)
    return (np.sqrt(np.sum(D * D, axis=0)) / np.sqrt(np.sum(np.asarray(R).astype(LD) ** 2, axis=0))).astype(np.double)


# ---- the iteration --------------------------------------------------------------------------------------------------------------
def reference_cg(G, B, pre=None, X0=None, rtol=1e-10, maxiter=2000):
    """`_matrix_free.pcg`, statement by statement, in longdouble.  Returns (X, iterations, rel)."""
    GL = np.asarray(G).astype(LD)
    B2 = np.asarray(B).astype(LD).reshape(GL.shape[0], -1)
    pr.longdouble_ok(GL.shape[0], GL.shape[0])           # a row of G P: n 2^-64 here against the n u of a float64 evaluation
    X = np.zeros_like(B2) if X0 is None else np.asarray(X0).astype(LD).reshape(B2.shape)
    R = B2 - GL @ X if X0 is not None else B2.copy()
    bn = np.sqrt(np.sum(B2 * B2, axis=0))
    bn[bn == 0] = 1
    Z = pre.solve(R) if pre is not None else R
    P = Z.copy()
    rz = np.sum(R * Z, axis=0)
    it, rel = 0, np.sqrt(np.sum(R * R, axis=0)) / bn
    while it < maxiter and np.any(rel > rtol):
        Q = GL @ P
        pq = np.sum(P * Q, axis=0)
        active = (rel > rtol) & (pq > 0)
        alpha = np.where(active, rz / np.where(pq > 0, pq, LD(1)), LD(0))
        X = X + alpha * P
        R = R - alpha * Q
        Z = pre.solve(R) if pre is not None else R
        rz_new = np.sum(R * Z, axis=0)
        beta = np.where(active, rz_new / np.where(rz != 0, rz, LD(1)), LD(0))
        P = Z + beta * P
        rz = rz_new
        rel = np.sqrt(np.sum(R * R, axis=0)) / bn
        it += 1
    return X, it, rel.astype(np.double)


def true_residual(G, X, B):
    """||B - G X|| / ||B|| per column, longdouble."""
    GL = np.asarray(G).astype(LD)
    B2 = np.asarray(B).astype(LD).reshape(GL.shape[0], -1)
    D = B2 - GL @ np.asarray(X).astype(LD).reshape(B2.shape)
    bn = np.sqrt(np.sum(B2 * B2, axis=0))
    bn[bn == 0] = 1
    return (np.sqrt(np.sum(D * D, axis=0)) / bn).astype(np.double)


def build_preconditioner(G, rank):
    """The class under test on the dense matrix.  Returns (preconditioner, pivots in their order)."""
    from linpde_gp_amd.randprocs import _matrix_free as mfree
    dense = DenseGram(G)
    pre = mfree.PivotedCholeskyPreconditioner(dense, rank)
    return pre, list(dense.rows_asked)


@functools.lru_cache(maxsize=None)
def reference_iterations(kernel, n, noise, rank, columns=COLUMNS):
    """Iterations of the longdouble CG with the class's preconditioner (rank setting `rank`) on the case: (count, worst rel)."""
    c = case(kernel, n, noise, columns)
    pre, _ = build_preconditioner(c.G, rank)
    _, it, rel = reference_cg(c.G, c.B, ReferencePreconditioner(pre.L, pre.delta), rtol=c.rtol)
    return it, float(np.max(rel))
