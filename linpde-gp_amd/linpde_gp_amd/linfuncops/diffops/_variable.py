"""Differential operators with variable coefficients: `L = sum_a f_a(x) D_a`.

Every other operator of this package has constant coefficients and therefore ONE canonical form, a coefficient map
(`coefficients_dict`).  A coefficient that depends on the point -- a diffusivity `-(a(x) u')' = -a u'' - a' u'`, advection
by a velocity field `v(x) . grad u`, a reaction term `c(x) u` -- multiplies every Gram entry by a value that depends on its
row and on its column, which no coefficient map can express.  `VariableCoefficientOperator` keeps the operator as a short
list of terms `(f_a, D_a)`, `D_a` with constant coefficients and `f_a` a scalar function of the point; the Gram and cross
blocks of an observation `L[u](X)` are then

    G[i, j] = sum_{a, b}  f_a(x_i) (D_a k D_b'^*)(x_i, x'_j) g_b(x'_j),

assembled by one fused kernel (`lpgp_gram_assemble_weighted`, csrc/assemble.hip) from ordinary descriptors, one per pair.
The reference has no counterpart: the weights of its `WeightedLaplacian` are constants.
"""

from __future__ import annotations

import numpy as np

from ..._lib import MAXW
from ...functions import Function, apply_coefficients
from .._linfuncop import LinearFunctionOperator
from ._operators import _as_shape

FEATURE = "variable-coefficient operators (`VariableCoefficientOperator`)"


class WeightedSum(Function):
    """`x -> sum_a f_a(x) g_a(x)` (`f_a` None: the constant 1): a variable-coefficient operator applied to a function."""

    def __init__(self, weights, fns):
        self._weights, self._fns = tuple(weights), tuple(fns)
        super().__init__(self._fns[0].input_shape, ())

    def _evaluate(self, x):
        out = 0.0
        for f, g in zip(self._weights, self._fns):
            v = np.asarray(g(x), dtype=np.double)
            out = out + (v if f is None else np.asarray(f(x), dtype=np.double) * v)
        return out


class VariableCoefficientOperator(LinearFunctionOperator):
    """`sum_a f_a(x) D_a` on functions with input shape `input_shape`.

    `terms`: a sequence of `(f, D)`; `D` a constant-coefficient `LinearDifferentialOperator` (or any operator with a
    `coefficients_dict`), `f` a `functions.Function` of that input shape with scalar output, or None for the constant 1.
    Terms that share the same `f` OBJECT are merged (their coefficient maps add).  At most `LPGP_MAXW` = 4 terms remain;
    more raise `NotImplementedError`.

    Algebra: `-L`, `c * L` for a scalar `c`, `L + M` and `L - M` with a constant-coefficient operator or another
    `VariableCoefficientOperator` (the result is again one flat term list).  There is deliberately no sugar on
    `Function.__mul__`.

    `L(m)` for a function `m` is `sum_a f_a . D_a(m)` through the closed-form derivatives of `functions.differentiate`
    (`NotImplementedError` where a derivative is missing).  `condition_on_observations(Y, X, L=L)` is supported on a dense,
    single-GPU prior or posterior; as a read-out (`L(posterior)`, `L(prior)`, `L(k)`) it raises `NotImplementedError`.
    """

    _variable_coefficients = True        # (what the constant-coefficient layers test for, without importing this module)

    def __init__(self, input_shape, terms):
        input_shape = _as_shape(input_shape)
        if len(input_shape) > 1:
            raise ValueError("only input shapes () and (d,) are supported")
        d = input_shape[0] if input_shape else 1
        merged: list = []                # [f, coefficient map]
        for term in terms:
            try:
                f, D = term
            except (TypeError, ValueError):
                raise TypeError("`terms` must be a sequence of pairs (f, D)") from None
            if f is not None:
                if not isinstance(f, Function):
                    raise TypeError(f"a coefficient must be a `functions.Function` or None, got {type(f).__name__}")
                if tuple(f.input_shape) != input_shape or tuple(f.output_shape) != ():
                    raise ValueError(f"a coefficient function must map input shape {input_shape} to a scalar, got "
                                     f"{tuple(f.input_shape)} -> {tuple(f.output_shape)}")
            if isinstance(D, VariableCoefficientOperator):
                raise TypeError("the operator of a term must have constant coefficients (add two `VariableCoefficientOperator`s instead)")
            if not isinstance(D, LinearFunctionOperator):
                raise TypeError(f"the operator of a term must be a `LinearFunctionOperator`, got {type(D).__name__}")
            if tuple(D.input_domain_shape) != input_shape or tuple(D.input_codomain_shape) != ():
                raise ValueError(f"the operator of a term acts on input shape {tuple(D.input_domain_shape)}, expected {input_shape}")
            coeffs = {tuple(int(i) for i in mi): float(c) for mi, c in D.coefficients_dict().items()}
            if any(len(mi) != d for mi in coeffs):
                raise ValueError("the operator's multi-indices do not match the input dimension")
            for entry in merged:
                if entry[0] is f:
                    for mi, c in coeffs.items():
                        entry[1][mi] = entry[1].get(mi, 0.0) + c
                    break
            else:
                merged.append([f, dict(coeffs)])
        if not merged:
            raise ValueError("at least one term is required")
        if len(merged) > MAXW:
            raise NotImplementedError(f"{FEATURE}: at most {MAXW} terms with different coefficient functions are supported "
                                      f"(LPGP_MAXW), got {len(merged)}")
        self._terms = tuple((f, c) for f, c in merged)
        super().__init__(input_shapes=(input_shape, ()), output_shapes=(input_shape, ()))

    # -- introspection ------------------------------------------------------------------
    @property
    def terms(self):
        """`((f_a, {multi_index: coefficient}), ...)` after merging, in the order of first appearance; `f_a` None: 1."""
        return tuple((f, dict(c)) for f, c in self._terms)

    @property
    def coefficient_functions(self):
        return tuple(f for f, _ in self._terms)

    def coefficients_dict(self):
        raise NotImplementedError(f"{FEATURE} have no constant-coefficient form (`coefficients_dict`); use `terms`")

    def weights(self, X) -> np.ndarray:
        """`f_a(x_i)` as an array (number of terms, number of points) for points `X` of shape batch + input_shape."""
        X = np.asarray(X, dtype=np.double)
        batch = X.shape[: X.ndim - len(self._input_domain_shape)]
        n = int(np.prod(batch, dtype=int))
        W = np.ones((len(self._terms), n))
        for a, (f, _) in enumerate(self._terms):
            if f is not None:
                W[a] = np.broadcast_to(np.asarray(f(X), dtype=np.double), batch).reshape(-1)
        return W

    def __repr__(self):
        return f"VariableCoefficientOperator({len(self._terms)} terms on input shape {self._input_domain_shape})"

    # -- application --------------------------------------------------------------------
    def __call__(self, f, /, *, argnum: int = 0):
        if isinstance(f, Function):
            if tuple(f.input_shape) != self._input_domain_shape or tuple(f.output_shape) != ():
                raise ValueError(f"the operator acts on scalar functions with input shape {self._input_domain_shape}")
            return WeightedSum([w for w, _ in self._terms], [apply_coefficients(c, f) for _, c in self._terms])
        raise NotImplementedError(
            f"{FEATURE} can be conditioned on (`condition_on_observations(Y, X, L=...)`) and applied to a `Function`; as a "
            f"read-out of a {type(f).__name__} (`L(posterior)`, `L(prior)`, `L(k)`) they are not supported yet")

    # -- algebra ------------------------------------------------------------------------
    def _raw_terms(self):
        return [(f, _Coefficients(self._input_domain_shape, c)) for f, c in self._terms]

    def __rmul__(self, other):
        if np.ndim(other) == 0:
            s = float(other)
            return VariableCoefficientOperator(
                self._input_domain_shape,
                [(f, _Coefficients(self._input_domain_shape, {mi: s * c for mi, c in cs.items()})) for f, cs in self._terms])
        return NotImplemented

    def __neg__(self):
        return -1.0 * self

    def __add__(self, other):
        if isinstance(other, VariableCoefficientOperator):
            return VariableCoefficientOperator(self._input_domain_shape, self._raw_terms() + other._raw_terms())
        if isinstance(other, LinearFunctionOperator):
            return VariableCoefficientOperator(self._input_domain_shape, self._raw_terms() + [(None, other)])
        return NotImplemented

    def __radd__(self, other):
        if isinstance(other, LinearFunctionOperator):
            return VariableCoefficientOperator(self._input_domain_shape, [(None, other)] + self._raw_terms())
        return NotImplemented

    def __sub__(self, other):
        if isinstance(other, LinearFunctionOperator):
            return self + (-other)
        return NotImplemented

    def __rsub__(self, other):
        if isinstance(other, LinearFunctionOperator):
            return other + (-self)
        return NotImplemented


class _Coefficients(LinearFunctionOperator):
    """A constant-coefficient operator given by its coefficient map (the algebra above rebuilds term lists from maps)."""

    def __init__(self, input_shape, coeffs):
        super().__init__(input_shapes=(input_shape, ()), output_shapes=(input_shape, ()))
        self._coeffs = dict(coeffs)

    def coefficients_dict(self):
        return dict(self._coeffs)
