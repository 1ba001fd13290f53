"""Dense NumPy/SciPy reference for observations through a matrix, `A @ L` (test-only).

An observation block is plain data: points X, a coefficient map D of the operator under the matrix (as in `oracle.covfuncs`), and
a dense matrix A of shape (rows, points), or None for plain point functionals.  A block of the Gram matrix is

    A0 @ LkL(D0, D1)(X0, X1) @ A1.T

from the oracle's constant-coefficient block; the posterior is the Cholesky one of `oracle/gp.py`.  The two problems of
tests/test_gpu_mixed.py are built here once per session, in the oracle's data and as the package's objects.
"""
from dataclasses import dataclass, field

import numpy as np
import scipy.linalg

from oracle import covfuncs as ocf
from oracle import gp as ogp

from _varcoef_reference import lp_coeffs, lp_kernel


def block(kernel, D0, D1, X0, X1, A0=None, A1=None):
    """Reference block A0 K A1^T, its envelope |A0| |K| |A1|^T and absw = (|A0| 1) max|K| (|A1| 1)^T (for error bounds)."""
    K = ocf.LkL(kernel, D0, D1, X0, X1)
    A0 = np.eye(X0.shape[0]) if A0 is None else np.asarray(A0, dtype=np.double)
    A1 = np.eye(X1.shape[0]) if A1 is None else np.asarray(A1, dtype=np.double)
    out = A0 @ K @ A1.T
    env = np.abs(A0) @ np.abs(K) @ np.abs(A1).T
    absw = np.outer(np.abs(A0).sum(axis=1), np.abs(A1).sum(axis=1)) * np.max(np.abs(K))
    return out, env, absw


def stencil_block(kernel, D0, D1, X0, X1, idx0, w0, idx1, w1):
    """The literal double loop over the stencils of an ELL table pair: entry (r, c) = sum_a sum_b w0[r,a] w1[c,b] K[idx0[r,a], idx1[c,b]]."""
    K = ocf.LkL(kernel, D0, D1, X0, X1)
    out = np.zeros((idx0.shape[0], idx1.shape[0]))
    for r in range(idx0.shape[0]):
        for c in range(idx1.shape[0]):
            s = 0.0
            for a in range(idx0.shape[1]):
                for b in range(idx1.shape[1]):
                    s += w0[r, a] * w1[c, b] * K[idx0[r, a], idx1[c, b]]
            out[r, c] = s
    return out


def dense_of(idx, w, npts):
    """The matrix whose rows the table (idx, w) holds (padding slots add their exact zeros)."""
    A = np.zeros((idx.shape[0], npts))
    np.add.at(A, (np.repeat(np.arange(idx.shape[0]), idx.shape[1]), idx.reshape(-1)), w.reshape(-1))
    return A


@dataclass
class Obs:
    X: np.ndarray                 # (n, d)
    D: dict                       # {multi_index: c}
    A: "np.ndarray | None"        # (rows, n) or None
    Y: np.ndarray                 # (rows,)
    noise: float = 0.0            # variance

    @property
    def rows(self):
        return self.X.shape[0] if self.A is None else self.A.shape[0]


@dataclass
class Reference:
    kernel: list
    obs: list
    G: np.ndarray = field(init=False)
    chol: np.ndarray = field(init=False)
    r: np.ndarray = field(init=False)
    w: np.ndarray = field(init=False)

    def __post_init__(self):
        rows = [[block(self.kernel, oi.D, oj.D, oi.X, oj.X, oi.A, oj.A)[0] for oj in self.obs] for oi in self.obs]
        G = np.block(rows)
        G = 0.5 * (G + G.T)
        off = 0
        for o in self.obs:
            G[off:off + o.rows, off:off + o.rows] += o.noise * np.eye(o.rows)
            off += o.rows
        self.G = G
        self.chol = scipy.linalg.cholesky(G, lower=True)
        self.r = np.concatenate([np.asarray(o.Y, dtype=np.double) for o in self.obs])        # zero prior mean
        self.w = scipy.linalg.cho_solve((self.chol, True), self.r)

    def cross(self, Xt):
        d = Xt.shape[1]
        return np.concatenate([block(self.kernel, ocf.identity(d), o.D, Xt, o.X, None, o.A)[0] for o in self.obs], axis=1)      # (M, N)

    def predict(self, Xt):
        K = self.cross(Xt)
        V = scipy.linalg.solve_triangular(self.chol, K.T, lower=True)
        d = Xt.shape[1]
        return K @ self.w, ocf.k_diag(self.kernel, ocf.identity(d), ocf.identity(d), Xt) - ogp.colsumsq(V)

    def cov(self, Xt):
        K = self.cross(Xt)
        V = scipy.linalg.solve_triangular(self.chol, K.T, lower=True)
        d = Xt.shape[1]
        return ocf.LkL(self.kernel, ocf.identity(d), ocf.identity(d), Xt, Xt) - V.T @ V

    def refined(self, Xt):
        """Mean, variance (`oracle.gp.refined_posterior`: long-double residuals) and representer weights refined the same way."""
        n, d = self.G.shape[0], Xt.shape[1]
        post = ogp.Posterior(self.kernel, [ogp.ObsBlock(np.zeros((n, d)), ocf.identity(d), self.r)], 0.0, self.G, self.chol, self.w)
        mean, var = ogp.refined_posterior(post, Xt, K=self.cross(Xt))
        Gl, w = self.G.astype(np.longdouble), self.w.astype(np.longdouble)
        for _ in range(12):
            w = w + scipy.linalg.cho_solve((self.chol, True), (self.r.astype(np.longdouble) - Gl @ w).astype(np.double))
        return mean, var, np.asarray(w, dtype=np.double)


# ---- quadrature ---------------------------------------------------------------------------------------------------------
def gauss_cells_1d(edges, npts):
    """Gauss-Legendre points of every cell [edges[i], edges[i+1]] and the matrix of cell AVERAGES (cells, cells * npts)."""
    t, wt = np.polynomial.legendre.leggauss(npts)
    lo, hi = edges[:-1], edges[1:]
    X = (0.5 * (lo + hi)[:, None] + 0.5 * (hi - lo)[:, None] * t[None, :]).reshape(-1)
    A = np.zeros((lo.size, lo.size * npts))
    for c in range(lo.size):
        A[c, c * npts:(c + 1) * npts] = 0.5 * wt
    return X, A


# ---- the two problems ---------------------------------------------------------------------------------------------------
BOUNDARY_NOISE = 1e-6


def problem_1d(order):
    """Cell averages of -u'' over 140 cells of [-1, 1] by 3-point Gauss-Legendre (420 points, 140 rows, no noise), two noisy boundary
    values, Matern-7/2, lengthscale 0.6; u = sin 2x.  `order`: "boundary first" or "cells first"."""
    kernel = [(1.0, [("matern", 3.5, 0.6)])]
    x, A = gauss_cells_1d(np.linspace(-1, 1, 141), 3)
    f = A @ (4 * np.sin(2 * x))
    cells = Obs(x[:, None], {(2,): -1.0}, A, f)
    bd = [Obs(np.array([[b]]), ocf.identity(1), None, np.array([np.sin(2 * b)]), BOUNDARY_NOISE) for b in (-1.0, 1.0)]
    return kernel, (bd + [cells] if order == "boundary first" else [cells] + bd), np.linspace(-0.97, 0.99, 33)[:, None]


def problem_2d():
    """Averages of -Lap u over 12 x 12 cells of [-1, 1]^2 by 2 x 2 Gauss (576 points, 144 rows), four noisy boundary edges of 15
    values, Matern-5/2 x Matern-5/2 with lengthscale 1, 50 scattered test points; u = sin x cos y."""
    kernel = [(1.0, [("matern", 2.5, 1.0), ("matern", 2.5, 1.0)])]
    x1, A1 = gauss_cells_1d(np.linspace(-1, 1, 13), 2)
    Xq = np.stack(np.meshgrid(x1, x1, indexing="ij"), axis=-1).reshape(-1, 2)
    A = np.kron(A1, A1)
    u = lambda X: np.sin(X[:, 0]) * np.cos(X[:, 1])
    cells = Obs(Xq, {(2, 0): -1.0, (0, 2): -1.0}, A, A @ (2 * u(Xq)))
    g = np.linspace(-1, 1, 15)
    edges = [np.stack([np.full(15, -1.0), g], 1), np.stack([np.full(15, 1.0), g], 1), np.stack([g, np.full(15, -1.0)], 1), np.stack([g, np.full(15, 1.0)], 1)]
    obs = [Obs(E, ocf.identity(2), None, u(E), BOUNDARY_NOISE) for E in edges] + [cells]
    return kernel, obs, np.random.default_rng(50).uniform(-1, 1, (50, 2))


# ---- the same data as the package's objects -----------------------------------------------------------------------------
def lp_functional(lp, o, scalar_input=False, sparse=False):
    """The package's functional of an observation block: `A @ (ev @ D)`, `ev @ D`, or plain evaluation."""
    d = o.X.shape[1]
    shape = () if scalar_input else (d,)
    L = lp.linfunctls._EvaluationFunctional(shape, (), o.X[:, 0] if scalar_input else o.X)
    if o.D != ocf.identity(d):
        L = L @ lp_coeffs(o.D, scalar_input)
    if o.A is None:
        return L
    if sparse:
        import scipy.sparse
        return scipy.sparse.csr_matrix(o.A) @ L
    return o.A @ L


def condition(lp, kernel, obs, scalar_input=False, sparse=False):
    """The chain of conditionings through the public interface."""
    d = obs[0].X.shape[1]
    u = lp.GaussianProcess(lp.functions.Zero(() if scalar_input else (d,)), lp_kernel(lp, kernel))
    for o in obs:
        b = lp.randvars.Normal(np.zeros(o.rows), np.full(o.rows, o.noise)) if o.noise else None
        u = u.condition_on_observations(np.asarray(o.Y), L=lp_functional(lp, o, scalar_input, sparse), b=b)
    return u
