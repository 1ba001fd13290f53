"""Helpers shared by the backward-error suites (test_gpu_potrf_backward.py, test_gpu_predict_backward.py, test_gpu_dist_backward.py): long-double products
in row slabs, the scaled backward error of a Cholesky factor, block rows appended as a conditioning builds them, and the
restoring of schedule options.  A plain module the suites import, not a conftest."""
import contextlib

import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble
PROBES = 8
FULL_MAX = 512

_cache = {}


def mv(M, X):
    """M @ X in long double, in row slabs (n = 8320 would need 1 GB as one long-double array)."""
    out = np.empty((M.shape[0], X.shape[1]), dtype=LD)
    for i in range(0, M.shape[0], 1024):
        out[i:i + 1024] = M[i:i + 1024].astype(LD) @ X
    return out


def mtv(M, X):
    """M^T @ X in long double."""
    out = np.zeros((M.shape[1], X.shape[1]), dtype=LD)
    for i in range(0, M.shape[0], 1024):
        out += M[i:i + 1024].astype(LD).T @ X[i:i + 1024]
    return out


def scale(A):
    return 1.0 / np.sqrt(np.diag(A))


def probes(n):
    return np.random.default_rng(n).standard_normal((n, PROBES)).astype(LD)


def backward_error(A, L):
    """max |S (A - L L^T) S| (n <= FULL_MAX) or max |S (A - L L^T) S X| / max_j ||X_j||_2 on the probes X; S = diag(A)^{-1/2}."""
    n = A.shape[0]
    s = scale(A).astype(LD)
    if n <= FULL_MAX:
        Ls = L.astype(LD) * s[:, None]
        R = A.astype(LD) * s[:, None] * s[None, :] - Ls @ Ls.T
        return float(np.max(np.abs(R)))
    X = probes(n)
    key = ("AX", id(A), n)
    if key not in _cache:
        _cache[key] = s[:, None] * mv(A, s[:, None] * X)
    AX = _cache[key]
    R = AX - s[:, None] * mv(L, mtv(L, s[:, None] * X))
    return float(np.max(np.abs(R)) / np.max(np.sqrt(np.sum(X * X, axis=0))))


def solve_backward_error(A, x, b):
    """Normwise backward error of x as a solution of A x = b, per the solve check of test_gpu_potrf_backward.py:
    max |A x - b| / (||A||_inf max |x| + max |b|), the residual in long double."""
    x, b = x.reshape(A.shape[0], -1), b.reshape(A.shape[0], -1)
    r = mv(A, x.astype(LD)) - b.astype(LD)
    nA = float(np.max(np.sum(np.abs(A), axis=1)))
    return float(np.max(np.abs(r))) / (nA * float(np.max(np.abs(x))) + float(np.max(np.abs(b))))


def row_scaled_distance(A, L1, L2):
    """max |diag(A)^{-1/2} (L1 - L2)|: the distance of two factors of A that the append test of test_gpu_potrf_backward.py bounds."""
    return float(np.max(np.abs((L1 - L2) * scale(A)[:, None])))


def matern52(n, rng):
    X = rng.uniform(0, 1, (n, 2))
    r = np.sqrt(5.0) * np.sqrt(np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=-1)) / 0.3
    return (1 + r + r * r / 3) * np.exp(-r) + 1e-8 * np.eye(n)


# appended block rows: a Matern-5/2 Gram on scattered 2-D points plus diagonal noise of three kinds
NOISE = {"m": lambda rng, n: np.ones(n),                                  # well conditioned
         "b": lambda rng, n: np.full(n, 1e-8),                            # condition ~1e9
         "s": lambda rng, n: 10.0 ** rng.uniform(-6, 6, n)}               # rows scaled over twelve decades


def gram_points(kind, n):
    rng = np.random.default_rng(7 * n + ord(kind))
    return rng.uniform(0, 1, (n, 2)), NOISE[kind](rng, n)


class Appender:
    """Appends block rows of the Gram of `X` plus diag(`noise`) to a GramMatrix as a conditioning does: all blocks of the new
    row assembled on the device, then the noise (plus `extra`, a diagonal perturbation of the new block) added.
    `capacity`: the matrix's capacity hint in rows (default: the rows of `X`)."""

    def __init__(self, ctx, X, noise, capacity=None):
        from linpde_gp_amd import _engine
        from linpde_gp_amd.randprocs import covfuncs
        self.ctx, self.X, self.noise = ctx, X, noise
        self.kd = covfuncs.Matern((2,), nu=2.5, lengthscales=0.3).lower()
        self.mat = _engine.GramMatrix(ctx, X.shape[0] if capacity is None else capacity)
        self.pts = []

    def add(self, nb, extra=None):
        from linpde_gp_amd import _engine
        mat, lo = self.mat, self.mat.n
        bi = mat.add_block(nb)
        P = _engine.Points(self.ctx, np.ascontiguousarray(self.X[lo:lo + nb]))
        self.pts.append(P)
        for bj in range(bi):
            mat.assemble(self.kd, P, self.pts[bj], bi, bj)
        mat.assemble(self.kd, P, None, bi, bi)
        v = self.noise[lo:lo + nb].copy()
        if extra is not None:
            v += extra
        mat.add_diag(bi, v)
        return bi

    def drop(self, nblocks, truncate=False):
        """Rollback to `nblocks` blocks (pop_block of the last, or truncate)."""
        if truncate:
            self.mat.truncate(nblocks)
        else:
            assert self.mat.num_blocks == nblocks + 1
            self.mat.pop_block()
        del self.pts[nblocks:]


@contextlib.contextmanager
def restored(ctx, keys):
    """Yields apply(dict), which sets options; every option of `keys` is restored on exit, profiling switched off."""
    saved = {k: ctx.get_option(k) for k in keys}

    def apply(row):
        for k, v in row.items():
            ctx.set_option(k, v)
    try:
        yield apply
    finally:
        ctx.profile_enable(False)
        for k, v in saved.items():
            ctx.set_option(k, v)
