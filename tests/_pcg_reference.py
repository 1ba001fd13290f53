"""High-precision reference of ONE iteration of the preconditioned conjugate gradients of `csrc/pcg.hip` (`lpgp_pcg_start`,
`lpgp_pcg_step`), the running error bounds the device is held to, and the inputs of the suites (test_pcg_reference.py on the CPU,
test_gpu_pcg_kernels.py on the device).  A plain module, not a conftest: NumPy, `fractions` and `math.fsum`, no device code.

The specification is the host loop `randprocs/_matrix_free.pcg`; `start` and `step` below are that loop, statement by statement,
with the state explicit (`rz`, `bn`, `rel`, `active`) and the product Q = G P an INPUT of the step, as it is on the device.  The
preconditioner is  Z = (R - L^T (S (L R))) / delta  with S used as given (not symmetrised: a transposed index shows).

Arithmetic.  Every sum over the n rows (column dots, the rows of L R) is the exact sum of exact products -- Dekker's two-product
on the float64 parts of the operands, `math.fsum` over all of them -- rounded once to `np.longdouble` (2^-64).  Vectors are carried
in `np.longdouble`; one is exactly the sum of two float64 arrays, which is how it enters the exact dots.  The short sums over the
rank of the preconditioner are plain `np.longdouble`, where `longdouble_ok` asserts that their own bound,
terms * 2^-64 * sum|a b|, is below 1/100 of the tolerance they serve.

Bounds.  None is measured; all follow from the depth of the summations in the kernels, u = 2^-53:
  column dot        (ceil(n / 32768) + 8 + 128 + 1) u sum|a_i b_i|      per-thread chain, 256-wide tree, serial sum of G = 128
                                                                      partials, the fma
  preconditioner    c u (|R| + |L|^T |S| |L| |R|) / delta componentwise, c = (ceil(n / 256) + 8) + 2 rank + 4
  alpha, beta, rel  first-order propagation of the dot bounds, one u per operation
  X, R, P           |d alpha| |P| + u (|alpha P| + |X|) and its analogues; an error of R goes through |M^-1| into Z
and the whole is doubled for the second-order terms.  (The bounds themselves are evaluated in float64: their own relative error,
n u, is immaterial.)"""
import dataclasses
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53            # unit roundoff of float64
DOT_STRIDE = 128 * 256    # rows one trip of pcg_dot_kernel's grid-stride loop covers (G = 128 workgroups of 256 threads)
COND_MAX = 100.0          # cap on sum|a b| / |sum a b| of every column dot of a run: a condition on the inputs, not a measurement


def dot_depth(n):
    return -(-n // DOT_STRIDE) + 8 + 128 + 1


def precond_depth(n, rank):
    return (-(-n // 256) + 8) + 2 * rank + 4


def longdouble_ok(terms, depth):
    """A `np.longdouble` sum of `terms` products stands in for an exact one where its bound is below 1/100 of `depth` u."""
    assert np.finfo(LD).nmant >= 63, "np.longdouble is not the 80-bit extended format here"
    assert terms * 2.0 ** -64 <= depth * U / 100, (terms, depth)


# ---- exact sums ---------------------------------------------------------------------------------------------------------------
_SPLITTER = 134217729.0   # 2^27 + 1


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp; float64, no over- or underflow at the magnitudes of these tests)"""
    p = a * b
    t = _SPLITTER * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLITTER * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _parts(A):
    """float64 arrays whose exact sum is A (one for float64 input, two for `np.longdouble`)"""
    A = np.asarray(A)
    if A.dtype != LD:
        return (np.asarray(A, dtype=np.float64),)
    hi = A.astype(np.float64)
    lo = (A - hi).astype(np.float64)          # exact: at most 12 significant bits are left
    return (hi, lo) if lo.any() else (hi,)


def _fsum2(terms):
    """the exact sum of a list of floats, to 2^-64"""
    hi = math.fsum(terms)
    terms.append(-hi)
    return LD(hi) + LD(math.fsum(terms))


def coldot(A, B):
    """Column dots of two n x m blocks (float64 or longdouble; an n x 1 operand broadcasts): (m,) longdouble."""
    A, B = np.asarray(A), np.asarray(B)
    terms = []
    for a in _parts(A):
        for b in _parts(B):
            terms.extend(_two_prod(a, b))
    T = np.stack(np.broadcast_arrays(*terms))
    return np.array([_fsum2(T[:, :, c].ravel().tolist()) for c in range(T.shape[2])], dtype=LD)


def colabs(A, B):
    """sum_i |a_i b_i| per column, float64"""
    return np.sum(np.abs(np.asarray(A, dtype=np.float64)) * np.abs(np.asarray(B, dtype=np.float64)), axis=0)


def fma_exact(a, b, c):
    """fl(a * b + c) with ONE rounding, element by element (scalars broadcast): `float(Fraction)` rounds correctly."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = np.empty(a.shape)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist(), c.reshape(-1).tolist())):
        flat[i] = float(Fraction(x) * Fraction(y) + Fraction(z))
    return out


# ---- the preconditioner ---------------------------------------------------------------------------------------------------------
class Preconditioner:
    """Z = (R - L^T (S (L R))) / delta;  L: rank x n, S: rank x rank as given, rank = 0: Z = R / delta."""

    def __init__(self, n, L, S, delta):
        self.n = int(n)
        self.L = np.zeros((0, self.n)) if L is None else np.asarray(L, dtype=np.float64).reshape(-1, self.n)
        self.rank = self.L.shape[0]
        self.S = np.zeros((0, 0)) if S is None else np.asarray(S, dtype=np.float64).reshape(self.rank, self.rank)
        self.delta = float(delta)
        self.depth = precond_depth(self.n, self.rank)

    def apply(self, R):
        R = np.asarray(R)
        RL = R.astype(LD)
        if self.rank == 0:
            return RL / LD(self.delta)
        longdouble_ok(2 * self.rank, self.depth)                    # S T and L^T U: `rank` products each
        T = np.stack([coldot(self.L[k][:, None], R) for k in range(self.rank)])
        Um = self.S.astype(LD) @ T
        return (RL - self.L.T.astype(LD) @ Um) / LD(self.delta)

    def absapply(self, D):
        """|M^-1| D = (D + |L|^T |S| |L| D) / delta"""
        D = np.asarray(D, dtype=np.float64)
        if self.rank == 0:
            return D / self.delta
        return (D + np.abs(self.L).T @ (np.abs(self.S) @ (np.abs(self.L) @ D))) / self.delta

    def bound(self, R):
        """componentwise bound of the device's own rounding in M^-1 R (not doubled)"""
        return self.depth * U * self.absapply(np.abs(np.asarray(R, dtype=np.float64)))

    def solve(self, R):
        """float64 evaluation with the interface of `PivotedCholeskyPreconditioner` (for `_matrix_free.pcg`)"""
        if self.rank == 0:
            return R / self.delta
        return (R - self.L.T @ (self.S @ (self.L @ R))) / self.delta


# ---- the iteration --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class State:
    X: np.ndarray
    R: np.ndarray
    Z: np.ndarray
    P: np.ndarray
    rz: np.ndarray          # <R, Z> per column
    bn: np.ndarray          # the norms the residuals are measured against
    rel: np.ndarray         # ||R|| / bn
    active: np.ndarray      # rel > rtol
    cond: dict              # sum|a b| / |sum a b| of the column dots taken to get here
    alpha: "np.ndarray | None" = None
    beta: "np.ndarray | None" = None


def bnorm(B):
    bn = np.linalg.norm(np.asarray(B, dtype=np.float64), axis=0)
    bn[bn == 0.0] = 1.0
    return bn


def _cond(A, B, s):
    with np.errstate(divide="ignore", invalid="ignore"):
        return colabs(A, B) / np.abs(s.astype(np.float64))


def _rel(R, bn, n):
    """rel = sqrt(<R, R>) / bn and its first-order bound given the componentwise bound dR of R (not doubled)"""
    rr = coldot(R, R)
    rel = np.sqrt(rr) / bn.astype(LD)
    return rr, rel


def _rel_bound(R, dR, rr, rel, n):
    e_rr = dot_depth(n) * U * colabs(R, R) + 2.0 * np.sum(np.abs(np.asarray(R, dtype=np.float64)) * dR, axis=0)
    rrf, relf = rr.astype(np.float64), rel.astype(np.float64)
    return np.where(rrf > 0.0, relf * (e_rr / np.where(rrf > 0.0, 2.0 * rrf, 1.0) + 2.0 * U), 0.0)


def state(pre, X, R, Z, P, bn, rtol):
    """The state of an iteration read back from somewhere: `rz` and `rel` recomputed accurately from R and Z."""
    rz = coldot(R, Z)
    rr, rel = _rel(R, np.asarray(bn), pre.n)
    return State(np.asarray(X), np.asarray(R), np.asarray(Z), np.asarray(P), rz, np.asarray(bn, dtype=np.float64), rel, rel > rtol,
                 {"rz": _cond(R, Z, rz), "rr": _cond(R, R, rr)})


def start(pre, R, bn, rtol, X=None):
    """Z = M^-1 R, P = Z, rz = <R, Z>, rel = ||R|| / bn.  Returns the state and the bounds {"Z", "P", "rel"} (doubled)."""
    R = np.asarray(R)
    Z = pre.apply(R)
    st = state(pre, np.zeros(R.shape, dtype=LD) if X is None else X, R, Z, Z.copy(), bn, rtol)
    dZ = pre.bound(R)
    return st, {"Z": 2.0 * dZ, "P": 2.0 * dZ, "rel": 2.0 * _rel_bound(R, 0.0 * dZ, coldot(R, R), st.rel, pre.n)}


def step(pre, st, Q, rtol):
    """One iteration of `_matrix_free.pcg` given Q = G P.  Returns the new state and the bounds {"X", "R", "Z", "P", "rel"} within
    which an evaluation with the summation depths of pcg.hip lies that starts from `st` with a stored rz within the dot bound
    of <R, Z> (doubled for the second-order terms)."""
    n = pre.n
    f = lambda A: np.asarray(A, dtype=np.float64)            # noqa: E731  (magnitudes for the bounds)
    cd = dot_depth(n) * U
    pq = coldot(st.P, Q)
    took = st.active & (pq > 0)
    alpha = np.where(took, st.rz / np.where(pq > 0, pq, LD(1)), LD(0))
    X = st.X.astype(LD) + alpha * st.P
    R = st.R.astype(LD) - alpha * Q
    Z = pre.apply(R)
    rzn = coldot(R, Z)
    beta = np.where(took, rzn / np.where(st.rz != 0, st.rz, LD(1)), LD(0))
    P = Z + beta * st.P
    rr, rel = _rel(R, st.bn, n)
    new = State(X, R, Z, P, rzn, st.bn, rel, rel > rtol, {"pq": _cond(st.P, Q, pq), "rz": _cond(R, Z, rzn), "rr": _cond(R, R, rr)},
                alpha, beta)
    # ---- bounds
    t = took.astype(np.float64)                               # (a column that takes no step is not touched: alpha = beta = 0 exactly)
    e_rz, e_pq = cd * colabs(st.R, st.Z), cd * colabs(st.P, Q)
    a, b = np.abs(f(alpha)), np.abs(f(beta))
    apq, arz = np.where(took, np.abs(f(pq)), 1.0), np.where(took, np.abs(f(st.rz)), 1.0)
    dalpha = t * ((e_rz + a * e_pq) / apq + U * a)
    dX = t * (dalpha * np.abs(f(st.P)) + U * (a * np.abs(f(st.P)) + np.abs(f(st.X))))
    dR = t * (dalpha * np.abs(f(Q)) + U * (a * np.abs(f(Q)) + np.abs(f(st.R))))
    dZ = pre.bound(R) + pre.absapply(dR)
    e_rzn = cd * colabs(R, Z) + np.sum(dR * np.abs(f(Z)) + np.abs(f(R)) * dZ, axis=0)
    dbeta = t * ((e_rzn + b * e_rz) / arz + U * b)
    dP = dZ + dbeta * np.abs(f(st.P)) + U * (b * np.abs(f(st.P)) + np.abs(f(Z)))
    return new, {"X": 2.0 * dX, "R": 2.0 * dR, "Z": 2.0 * dZ, "P": 2.0 * dP, "rel": 2.0 * _rel_bound(R, dR, rr, rel, n)}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the entries (0 / 0 counts as 0, anything / 0 as inf)"""
    err = np.abs(np.asarray(got).astype(LD) - np.asarray(ref).astype(LD)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
DELTA = 0.7
# (n, m, rank) of the local-error runs: below / above one 64-row pad, one 256-row block, the 32 768-row trip of the dots, all 256
# columns of the scalar kernel's single workgroup
STEP_SHAPES = [(63, 3, 2), (65, 5, 3), (257, 4, 5), (32768, 2, 3), (32769, 2, 3), (40001, 5, 3), (100, 256, 2)]
STEPS = 3


@dataclasses.dataclass
class Problem:
    n: int
    m: int
    rank: int
    d: np.ndarray
    W: np.ndarray
    L: np.ndarray
    S: np.ndarray
    B: np.ndarray
    delta: float = DELTA

    def matvec(self, V):
        """A V = d o V + W^T (W V) on the host, float64 (the result is an INPUT of the step: Q need not be exact)"""
        V = np.asarray(V, dtype=np.float64)
        return self.d[:, None] * V + self.W.T @ (self.W @ V)

    def preconditioner(self):
        return Preconditioner(self.n, self.L, self.S, self.delta)


def problem(n, m, rank, symmetric=True, seed=0):
    """d ~ U(0.5, 2), W (3 x n) / sqrt(n), L (rank x n) / sqrt(n), B standard normal, delta = 0.7.
    symmetric: S = C C^T scaled to ||L^T S L||_2 = 1/2, so M^-1 is positive definite and rz > 0.  Otherwise S is a plain random
    matrix / rank with S != S^T."""
    rng = np.random.default_rng([seed, n, m, rank, int(symmetric)])
    d = rng.uniform(0.5, 2.0, n)
    W = rng.standard_normal((3, n)) / np.sqrt(n)
    L = rng.standard_normal((rank, n)) / np.sqrt(n)
    B = rng.standard_normal((n, m))
    C = rng.standard_normal((rank, rank))
    if symmetric:
        S = C @ C.T
        if rank:
            S *= 0.5 / np.linalg.eigvalsh(C.T @ (L @ L.T) @ C)[-1]
    else:
        S = C / max(rank, 1)
    return Problem(n, m, rank, d, W, L, S, B)
