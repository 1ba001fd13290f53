"""Linear functionals on the hot path: point evaluation, optionally composed with a
differential operator.

Host mirror of
  `linfunctls/_linfunctl.py:14-129`   LinearFunctional (+ `@` with a function operator)
  `linfunctls/_evaluation.py:10-64`   _EvaluationFunctional (output = codomain shape, then
                                      batch shape; scalar-valued priors only here)
  `linfunctls/_dirac.py:10-45`        DiracFunctional (output = batch shape, then codomain shape:
                                      the same functional for the scalar-valued priors here)
  `linfunctls/_arithmetic.py:13-174`  Scaled / Sum / CompositeLinearFunctional and the operators
                                      `-L`, `a * L`, `L1 + L2`, `L1 - L2`, `L @ D`
                                      (`_linfunctl.py:76-112`), and `A @ L` with a matrix `A`
                                      (`_linfunctl.py:117-129`, `CompositeLinearFunctional(linop=A, ...)`)
Every functional of this path has the canonical form "point evaluation of `sum_a c_a d^a f` at
X": scaling multiplies the coefficient map, a sum over the SAME points adds the maps (a sum
over different point sets is not one observation block and raises NotImplementedError).
A leading matrix factor mixes these point functionals by its rows -- cell averages by quadrature, sensor averages, finite
differences of observed values -- and travels as a stencil table (`mixing()`, at most LPGP_MAXS = 32 non-zeros per row).
Closed-form integrals, L2 projections and weak forms are out of scope.
"""

from __future__ import annotations

import numpy as np

from ..linfuncops import LinearFunctionOperator


def _as_shape(shape):
    if isinstance(shape, (int, np.integer)):
        return (int(shape),)
    return tuple(int(s) for s in shape)


MAXS = 32        # LPGP_MAXS (include/lpgp.h): the most non-zeros a row of a leading matrix factor may have
_MATRIX = "a leading matrix factor (`A @ L`)"


def _is_sparse(A) -> bool:
    return hasattr(A, "tocsr") and hasattr(A, "toarray")


def _as_mixing_matrix(A):
    """`A` of `A @ L` as a 2-D float ndarray or a `scipy.sparse` CSR matrix; None if it is neither."""
    if _is_sparse(A):
        A = A.tocsr().astype(np.double)
        return A if A.ndim == 2 else None
    if isinstance(A, np.ndarray) and A.ndim == 2 and A.dtype.kind in "fiub":
        return np.asarray(A, dtype=np.double)
    return None


def _matrix_product(A2, A1):
    """`A2 @ A1` of two mixing matrices (sparse if either is)."""
    P = A2 @ A1
    return P.tocsr() if _is_sparse(P) else np.asarray(P, dtype=np.double)


def pack_rows(A):
    """(idx, w), both (q, S), of the rows of the mixing matrix `A` (`LinearFunctional.mixing`): the non-zeros of every row in
    column order (explicitly stored zeros of a sparse matrix are dropped), S = the longest row (at least 1), a shorter row
    padded with weight 0.0 and its first index, an empty row with index 0.  A row of more than LPGP_MAXS = 32 non-zeros raises
    `NotImplementedError`: dense mixing matrices belong on a GEMM path, which is not built."""
    if _is_sparse(A):
        A = A.tocsr().copy()
        A.sum_duplicates()
        A.eliminate_zeros()
        A.sort_indices()
        q = A.shape[0]
        indptr, cols, vals = np.asarray(A.indptr, dtype=np.int64), np.asarray(A.indices, dtype=np.int64), np.asarray(A.data, dtype=np.double)
        rows = np.repeat(np.arange(q, dtype=np.int64), np.diff(indptr))
    else:
        A = np.asarray(A, dtype=np.double)
        q = A.shape[0]
        rows, cols = np.nonzero(A)                 # (C order: by row, columns increasing)
        vals = A[rows, cols]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=q))]).astype(np.int64)
    counts = np.diff(indptr)
    longest = int(counts.max()) if q else 0
    if longest > MAXS:
        raise NotImplementedError(
            f"row {int(np.argmax(counts))} of {_MATRIX} has {longest} non-zeros, more than LPGP_MAXS = {MAXS}: dense mixing matrices "
            "(by GEMM) are not supported yet")
    S = max(longest, 1)
    first = np.zeros(q, dtype=np.int64)
    has = counts > 0
    first[has] = cols[indptr[:-1][has]]
    idx = np.repeat(first[:, None], S, axis=1)
    w = np.zeros((q, S))
    slot = np.arange(rows.size, dtype=np.int64) - indptr[:-1][rows]
    idx[rows, slot] = cols
    w[rows, slot] = vals
    return np.ascontiguousarray(idx, dtype=np.int32), w


class LinearFunctional:
    def __init__(self, input_shapes, output_shape):
        self._input_domain_shape = _as_shape(input_shapes[0])
        self._input_codomain_shape = _as_shape(input_shapes[1])
        self._output_shape = _as_shape(output_shape)

    @property
    def input_shapes(self):
        return (self._input_domain_shape, self._input_codomain_shape)

    @property
    def input_domain_shape(self):
        return self._input_domain_shape

    @property
    def input_codomain_shape(self):
        return self._input_codomain_shape

    @property
    def output_shape(self):
        return self._output_shape

    @property
    def output_size(self):
        return int(np.prod(self._output_shape, dtype=int))

    # canonical form used by the GPU path: evaluation points + operator coefficient map
    def points(self) -> np.ndarray:
        raise NotImplementedError

    def coefficients_dict(self) -> dict:
        raise NotImplementedError

    def device_points(self, ctx):
        """Device-resident evaluation points (reuses the handle of a `to_device` array)."""
        from .. import _engine

        return _engine.Points(ctx, self.points())

    # A functional built on a `diffops.VariableCoefficientOperator` has no coefficient map; its canonical form is
    # "point evaluation of  sum_a f_a(x) (D_a f)(x)  at X":  `variable_terms()` = (weights f_a(X) as an (A, n) array,
    # [coefficient map of D_a]), None for every constant-coefficient functional.
    def variable_terms(self):
        return None

    # A functional with a leading matrix factor, `A @ L` (`CompositeLinearFunctional(linop=A, ...)`), has the canonical form
    # "row r = sum_s w[r, s] * (point evaluation of sum_a c_a d^a f at X[idx[r, s]])":  `mixing()` = (idx, w), both of shape
    # (q, S), packed from the non-zeros of A's rows in column order, a shorter row padded with weight 0.0 and the row's first
    # index (an empty row: index 0); None for every functional without a matrix factor.
    def mixing(self):
        return None

    def __rmatmul__(self, other):
        A = _as_mixing_matrix(other)
        if A is None:
            return NotImplemented
        return CompositeLinearFunctional(linop=A, linfunctl=self, linfuncop=None)

    def __call__(self, f, /, *, argnum: int = 0):
        from ..functions import Function
        from ..randprocs import _gaussian_process as gps
        from ..randprocs import covfuncs

        if self.mixing() is not None and not isinstance(f, Function):
            return self._apply_mixed(f)
        if not isinstance(f, Function) and self.variable_terms() is not None:
            raise NotImplementedError(
                "a functional of a variable-coefficient operator (`VariableCoefficientOperator`) can be conditioned on and applied "
                f"to a `Function`; as a read-out of a {type(f).__name__} it is not supported yet")

        if isinstance(f, gps.ConditionalGaussianProcess):
            return gps.apply_linfunctl_to_conditional_gp(self, f)
        from ..randprocs._matrix_free import MatrixFreeConditionalGaussianProcess
        if isinstance(f, MatrixFreeConditionalGaussianProcess):
            # `L(posterior)` for a functional: the joint law of L[f] at the functional's points, through the matrix-free read-out
            from ..randvars import Normal
            view = f._with_test_operator(self)
            X = self.points()
            x = X if f.input_ndim else X[:, 0]
            return Normal(view.mean(x), view.cov.matrix(x))
        if isinstance(f, gps.GaussianProcess):
            return gps.apply_linfunctl_to_gp(self, f)
        if isinstance(f, covfuncs.CovarianceFunction):
            return covfuncs.ProcessVectorCrossCovariance(f, self, argnum=argnum)
        if isinstance(f, covfuncs.ProcessVectorCrossCovariance):
            return covfuncs.apply_linfunctl_to_pv_crosscov(self, f)
        if isinstance(f, Function):
            return self._apply_to_function(f)
        raise NotImplementedError(f"cannot apply {type(self).__name__} to {type(f).__name__}")

    def _apply_to_function(self, f):
        raise NotImplementedError

    def _apply_mixed(self, f):
        raise NotImplementedError

    def __matmul__(self, other):
        if isinstance(other, LinearFunctionOperator):
            return CompositeLinearFunctional(linfunctl=self, linfuncop=other)
        return NotImplemented

    # -- arithmetic (`_linfunctl.py:76-98`) --
    __array_ufunc__ = None

    def __neg__(self):
        return -1.0 * self

    def __add__(self, other):
        if isinstance(other, LinearFunctional):
            return SumLinearFunctional(self, other)
        return NotImplemented

    def __sub__(self, other):
        if isinstance(other, LinearFunctional):
            return self + (-other)
        return NotImplemented

    def __rmul__(self, other):
        if np.ndim(other) == 0:
            return ScaledLinearFunctional(linfunctl=self, scalar=other)
        return NotImplemented


class _EvaluationFunctional(LinearFunctional):
    def __init__(self, input_domain_shape, input_codomain_shape, X):
        input_domain_shape = _as_shape(input_domain_shape)
        input_codomain_shape = _as_shape(input_codomain_shape)
        self._X = np.asanyarray(X)
        nd = len(input_domain_shape)
        self._X_batch_shape = self._X.shape[: self._X.ndim - nd]
        if self._X.shape != self._X_batch_shape + input_domain_shape:
            raise ValueError(
                f"X has shape {self._X.shape}, expected batch shape + {input_domain_shape}")
        super().__init__(
            input_shapes=(input_domain_shape, input_codomain_shape),
            output_shape=input_codomain_shape + self._X_batch_shape,
        )

    @property
    def X(self):
        return self._X

    @property
    def X_batch_shape(self):
        return self._X_batch_shape

    def points(self) -> np.ndarray:
        d = self._input_domain_shape[0] if self._input_domain_shape else 1
        return np.ascontiguousarray(np.asarray(self._X, dtype=np.double).reshape(-1, d))

    def coefficients_dict(self):
        d = self._input_domain_shape[0] if self._input_domain_shape else 1
        return {(0,) * d: 1.0}

    def device_points(self, ctx):
        from .. import _engine

        return _engine.as_points(ctx, self._X, self.points())

    def _apply_to_function(self, f):
        res = np.asarray(f(self._X))
        if f.output_ndim > 0:
            res = np.moveaxis(res, res.ndim - f.output_ndim + np.arange(f.output_ndim), np.arange(f.output_ndim))
        return res


class DiracFunctional(_EvaluationFunctional):
    """Point evaluation with output layout batch shape + codomain shape (`_dirac.py:10-45`); for
    scalar-valued functions (the only ones on this path) the same functional as
    `_EvaluationFunctional`."""

    def __init__(self, input_domain_shape, input_codomain_shape, X):
        super().__init__(input_domain_shape, input_codomain_shape, X)
        self._output_shape = self._X_batch_shape + self._input_codomain_shape

    @property
    def X_batch_ndim(self):
        return len(self._X_batch_shape)

    def _apply_to_function(self, f):
        return np.asarray(f(self._X))


class ScaledLinearFunctional(LinearFunctional):
    """`scalar * linfunctl` (`_arithmetic.py:13-55`)."""

    def __init__(self, linfunctl: LinearFunctional, scalar):
        if np.ndim(scalar) != 0:
            raise ValueError("`scalar` must be a scalar")
        self._linfunctl = linfunctl
        self._scalar = float(scalar)
        super().__init__(input_shapes=linfunctl.input_shapes, output_shape=linfunctl.output_shape)

    @property
    def linfunctl(self):
        return self._linfunctl

    @property
    def scalar(self):
        return self._scalar

    def points(self):
        return self._linfunctl.points()

    def device_points(self, ctx):
        return self._linfunctl.device_points(ctx)

    def coefficients_dict(self):
        return {mi: self._scalar * c for mi, c in self._linfunctl.coefficients_dict().items()}

    def variable_terms(self):
        vt = self._linfunctl.variable_terms()
        return None if vt is None else (self._scalar * vt[0], vt[1])

    def mixing(self):
        return self._linfunctl.mixing()           # (the scalar sits in the coefficient map)

    def _apply_mixed(self, f):
        N = self._linfunctl(f)
        from ..randvars import Normal
        return Normal(self._scalar * np.asarray(N.mean), self._scalar ** 2 * np.asarray(N.cov))

    def _apply_to_function(self, f):
        return self._scalar * self._linfunctl(f)

    def __rmul__(self, other):
        if np.ndim(other) == 0:
            return ScaledLinearFunctional(linfunctl=self._linfunctl, scalar=float(other) * self._scalar)
        return NotImplemented


class SumLinearFunctional(LinearFunctional):
    """`L1 + L2 + ...` (`_arithmetic.py:58-89`).  On the MI355X path the summands must evaluate at
    the same points (e.g. a Robin condition `a * Id + b * d/dn` on one boundary grid)."""

    def __init__(self, *summands: LinearFunctional):
        if len(summands) < 1:
            raise ValueError("at least one summand is required")
        s0 = summands[0]
        if not all(s.input_shapes == s0.input_shapes for s in summands):
            raise ValueError("all summands must have the same input shapes")
        if not all(s.output_shape == s0.output_shape for s in summands):
            raise ValueError("all summands must have the same output shape")
        self._summands = tuple(summands)
        super().__init__(input_shapes=s0.input_shapes, output_shape=s0.output_shape)

    @property
    def summands(self):
        return self._summands

    def points(self):
        P = self._summands[0].points()
        for s in self._summands[1:]:
            Q = s.points()
            if Q.shape != P.shape or not np.array_equal(P, Q):
                raise NotImplementedError(
                    "a sum of functionals over different point sets is not one observation block; "
                    "condition on the summands' blocks separately")
        return P

    def device_points(self, ctx):
        self.points()
        return self._summands[0].device_points(ctx)

    def coefficients_dict(self):
        out: dict = {}
        for s in self._summands:
            for mi, c in s.coefficients_dict().items():
                out[mi] = out.get(mi, 0.0) + c
        return out

    def variable_terms(self):
        if any(s.variable_terms() is not None for s in self._summands):
            raise NotImplementedError("a sum of functionals with a variable-coefficient operator (`VariableCoefficientOperator`) among them "
                                      "is not supported: add the operators and evaluate the sum at the points")
        return None

    def mixing(self):
        if any(s.mixing() is not None for s in self._summands):
            raise NotImplementedError(f"a sum of functionals with {_MATRIX} among them is not supported: add the matrices over one "
                                      "point set and put the sum in front of one functional")
        return None

    def _apply_to_function(self, f):
        res = self._summands[0](f)
        for s in self._summands[1:]:
            res = res + s(f)
        return res


class CompositeLinearFunctional(LinearFunctional):
    """`linop @ linfunctl @ linfuncop` (`_arithmetic.py:92-174`) -- here: point evaluation of `linfuncop[f]`, optionally mixed by
    the rows of a matrix `linop` of shape (q, linfunctl.output_size): cell averages by quadrature, sensor averages, finite
    differences of observed values.  `linop`: a 2-D ndarray or a `scipy.sparse` matrix with at most LPGP_MAXS = 32 non-zeros per
    row; `A @ L` builds it.  The matrix acts on the flattened (C order) values of the inner functional, the output shape is (q,).
    A matrix in front of a functional that already has one is folded into it: `A2 @ (A1 @ L) == (A2 A1) @ L`."""

    def __init__(self, *, linfunctl: LinearFunctional, linfuncop: "LinearFunctionOperator | None" = None, linop=None):
        if linop is not None:
            A = _as_mixing_matrix(linop)
            if A is None:
                raise TypeError(f"`linop` must be a 2-D ndarray or a scipy.sparse matrix, got {type(linop).__name__}")
            if isinstance(linfunctl, CompositeLinearFunctional) and linfunctl._linop is not None:
                if linfuncop is not None:
                    raise NotImplementedError(f"a functional with {_MATRIX} may be composed with an operator only before the matrix is applied twice")
                if A.shape[1] != linfunctl.output_size:
                    raise ValueError(f"a matrix of shape {A.shape} does not match a functional with {linfunctl.output_size} outputs")
                A = _matrix_product(A, linfunctl._linop)
                linfunctl, linfuncop = linfunctl._linfunctl, linfunctl._linfuncop
            linop = A
        if linfuncop is not None and linfunctl.input_shapes != linfuncop.output_shapes:
            raise ValueError("shapes of the functional and the operator do not match")
        if linop is not None and linop.shape[1] != linfunctl.output_size:
            raise ValueError(f"a matrix of shape {linop.shape} does not match a functional with {linfunctl.output_size} outputs")
        self._linfunctl = linfunctl
        self._linfuncop = linfuncop
        self._linop = linop
        super().__init__(input_shapes=linfuncop.input_shapes if linfuncop is not None else linfunctl.input_shapes,
                         output_shape=linfunctl.output_shape if linop is None else (int(linop.shape[0]),))

    @property
    def linfunctl(self):
        return self._linfunctl

    @property
    def linfuncop(self):
        return self._linfuncop

    @property
    def linop(self):
        return self._linop

    def _unmixed(self) -> LinearFunctional:
        """The functional behind the matrix."""
        if self._linfuncop is None:
            return self._linfunctl
        return CompositeLinearFunctional(linfunctl=self._linfunctl, linfuncop=self._linfuncop)

    def mixing(self):
        if self._linop is None:
            return self._linfunctl.mixing()
        if self._linfunctl.mixing() is not None:
            raise NotImplementedError(f"{_MATRIX} in front of a functional that carries one inside a sum or a scaling is not supported")
        return pack_rows(self._linop)

    def __matmul__(self, other):
        if self._linop is not None and isinstance(other, LinearFunctionOperator):
            if self._linfuncop is not None:
                raise NotImplementedError(f"a functional with {_MATRIX} and an operator may not be composed with a further operator")
            return CompositeLinearFunctional(linop=self._linop, linfunctl=self._linfunctl, linfuncop=other)      # (A @ ev) @ D == A @ (ev @ D)
        return super().__matmul__(other)

    def __rmul__(self, other):
        if self._linop is not None and np.ndim(other) == 0:
            return CompositeLinearFunctional(linop=self._linop * float(other), linfunctl=self._linfunctl, linfuncop=self._linfuncop)
        return super().__rmul__(other)

    def _apply_mixed(self, f):
        """`(A @ L)(u)` for a prior or a posterior `u`: `Normal(A m, A Sigma A^T)` from the law `Normal(m, Sigma)` of `L(u)` on the
        functional's points; the two products with Sigma run on the device (`lpgp_gemm_host`)."""
        from .. import _engine
        from ..randprocs import _gaussian_process as gps
        from ..randprocs._matrix_free import MatrixFreeConditionalGaussianProcess
        from ..randvars import Normal

        if self._linop is None:
            return self._linfunctl._apply_mixed(f)
        if isinstance(f, MatrixFreeConditionalGaussianProcess):
            raise NotImplementedError(f"{_MATRIX} is not supported as a read-out of matrix-free posteriors")
        if not isinstance(f, gps.GaussianProcess):
            raise NotImplementedError(f"{_MATRIX} can be conditioned on, applied to a `Function` and read out of a Gaussian process; "
                                      f"applied to a {type(f).__name__} it is not supported")
        N = self._unmixed()(f)
        A = self._linop.toarray() if _is_sparse(self._linop) else self._linop
        ctx = f._state.ctx if isinstance(f, gps.ConditionalGaussianProcess) else _engine.default_context()
        n = A.shape[1]
        AS = _engine.gemm(ctx, A, np.asarray(N.cov, dtype=np.double).reshape(n, n))
        return Normal(A @ np.asarray(N.mean, dtype=np.double).reshape(n), _engine.gemm(ctx, AS, A, transb=True))

    def points(self):
        return self._linfunctl.points()

    def device_points(self, ctx):
        if self._linop is not None:
            # rows of a matrix over a tensor grid are no tensor grid: the block goes entry-wise, from the flattened points
            from .. import _engine
            return _engine.Points(ctx, self.points())
        return self._linfunctl.device_points(ctx)

    def coefficients_dict(self):
        inner = self._linfunctl.coefficients_dict()
        if self._linfuncop is None:
            return inner
        d = len(next(iter(inner)))
        if set(inner) != {(0,) * d}:
            raise NotImplementedError("only point evaluation may be composed with an operator")
        c0 = inner[(0,) * d]
        return {mi: c0 * c for mi, c in self._linfuncop.coefficients_dict().items()}

    def variable_terms(self):
        if self._linop is not None:
            if getattr(self._linfuncop, "_variable_coefficients", False) or self._linfunctl.variable_terms() is not None:
                raise NotImplementedError(f"a variable-coefficient operator (`VariableCoefficientOperator`) under {_MATRIX} is not supported")
            return None
        if self._linfuncop is None:
            return self._linfunctl.variable_terms()
        if not getattr(self._linfuncop, "_variable_coefficients", False):
            if self._linfunctl.variable_terms() is not None:
                raise NotImplementedError("a functional of a variable-coefficient operator may not be composed with a further operator")
            return None
        inner = self._linfunctl.coefficients_dict()
        d = len(next(iter(inner)))
        if set(inner) != {(0,) * d}:
            raise NotImplementedError("only point evaluation may be composed with an operator")
        X = self.points()
        W = self._linfuncop.weights(X if self._input_domain_shape else X[:, 0])
        return inner[(0,) * d] * W, [dict(c) for _, c in self._linfuncop.terms]

    def _apply_to_function(self, f):
        res = self._linfunctl(self._linfuncop(f) if self._linfuncop is not None else f)
        if self._linop is None:
            return res
        return np.asarray(self._linop @ np.asarray(res, dtype=np.double).reshape(-1))


__all__ = ["LinearFunctional", "_EvaluationFunctional", "DiracFunctional", "ScaledLinearFunctional",
           "SumLinearFunctional", "CompositeLinearFunctional"]
