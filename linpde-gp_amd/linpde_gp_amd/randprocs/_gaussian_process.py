"""`GaussianProcess` and `ConditionalGaussianProcess` -- orchestration of the hot path.

Host mirror of `randprocs/_gaussian_process/_conditional.py` of the reference:
  `from_observations`            :27-54    first conditioning
  `representer_weights`          :96-110
  `PriorPredictiveCrossCovariance` :112-175  kLas(x) = [(k L_j'^*)(x, X_j)]_j
  `Mean._evaluate`               :193-197  m(x) + kLas(x) @ w
  `CovarianceFunction._evaluate` :223-231  k(x,x') - kLas(x) G^{-1} kLas(x')^T
  `condition_on_observations`    :253-294  re-conditioning (Schur / block Cholesky)
  `_preprocess_observations`     :296-399  build L, validate X/Y/b, flatten C-order
  functional / operator read-outs :432-467
Same call signature, argument meaning and error behaviour; the arithmetic (Gram and
cross-covariance assembly, Cholesky, triangular solves, mean/variance reductions) runs in
liblpgp.so on the GPU and the factor stays resident in HBM: re-conditioning appends a
block row to the factor instead of nesting `BlockMatrix2x2` operators.
"""

from __future__ import annotations

import numpy as np

from .. import _engine, functions, linfunctls, randvars
from ..linfuncops import LinearFunctionOperator
from ..linfunctls import LinearFunctional
from . import covfuncs


class GaussianProcess:
    """Prior GP (probnum `randprocs.GaussianProcess` surface used by linpde-gp)."""

    def __init__(self, mean, cov):
        if not isinstance(mean, functions.Function):
            raise TypeError("`mean` must be a `functions.Function`")
        if not isinstance(cov, covfuncs.CovarianceFunction):
            raise TypeError("`cov` must be a `CovarianceFunction`")
        if mean.input_shape != cov.input_shape:
            raise ValueError(
                f"mean and covariance function disagree on the input shape: "
                f"{mean.input_shape} != {cov.input_shape}")
        if mean.output_shape != ():
            raise NotImplementedError("multi-output GPs are out of scope of the MI355X path")
        self._mean = mean
        self._cov = cov

    @property
    def mean(self):
        return self._mean

    @property
    def cov(self):
        return self._cov

    @property
    def input_shape(self):
        return self._mean.input_shape

    @property
    def input_ndim(self):
        return len(self._mean.input_shape)

    @property
    def output_shape(self):
        return ()

    def _flat(self, x):
        x = np.asarray(x, dtype=np.double)
        batch = x.shape[: x.ndim - self.input_ndim]
        d = max(int(np.prod(self.input_shape, dtype=int)), 1)
        return np.ascontiguousarray(x.reshape(-1, d)), batch

    def __call__(self, x) -> randvars.Normal:
        X, batch = self._flat(x)
        if len(batch) != 1:
            raise ValueError("`GaussianProcess.__call__` needs inputs of shape (N,) + input_shape")
        return randvars.Normal(self.mean(x), self.cov.matrix(x))

    def var(self, x):
        return self.cov(x, None)

    def std(self, x):
        return np.sqrt(np.maximum(self.var(x), 0.0))


    def sample(self, rng, x, size=(), *, damping=None):
        """Joint draws of the process at the points `x` (probnum `RandomProcess.sample(rng, args, size)`).

        `x` has shape batch + input_shape, the result shape size + batch; `size` is an int or a tuple, `size=()` gives one
        draw of shape batch.  THE RANDOM STREAM IS PART OF THE CONTRACT: exactly one call
        `z = rng.standard_normal(size + (M,))` with M = prod(batch), the points flattened in C order, and
        `draw[s] = mean(x) + C z[s]` with the lower Cholesky factor `C C^T = k(x, x) + delta I`,
        `delta = damping * k(x_0, x_0)` (the prior variance: the knob is scale-free; default `lp.config.sample_damping`).
        Draws are therefore reproducible from a seed.  The covariance is assembled, factored (`lpgp_potrf`) and multiplied
        (`lpgp_mat_factor_matmul`) on the device; the factor of the last point set is kept, so further draws at the same
        points cost one product.  Raises `ValueError` for `damping < 0`, `np.linalg.LinAlgError` (naming the damping) if
        the damped covariance does not factor."""
        size = _sample_size(size)
        damping = _sample_damping(damping)
        X, batch = _sample_points(self, x)
        M = X.shape[0]
        z = np.asarray(rng.standard_normal(size + (M,)), dtype=np.double)
        if z.shape != size + (M,):
            raise ValueError(f"`rng.standard_normal` returned shape {z.shape}, expected {size + (M,)}")
        if M == 0:
            return np.empty(size + batch)
        ctx = _sample_context()
        lowered = self.cov.lower()
        delta = damping * _engine.kernel_diag(ctx, lowered)
        hit = _cached_factor(self, X, delta, None)
        if hit is None:
            mean = np.array(np.broadcast_to(np.asarray(self.mean(x), dtype=np.double), batch), dtype=np.double).reshape(-1)
            S = _engine.GramMatrix(ctx, capacity_hint=M)
            S.add_block(M)
            S.assemble(lowered, _engine.Points(ctx, X), None, 0, 0)
            _factor_damped(S, delta, damping)
            self._sample_cache = ((_engine.option_epoch(), delta, None), X.copy(), S, mean)
            hit = (S, mean)
        return _draws(hit[0], hit[1], z, size, batch)

    def condition_on_observations(self, Y, X=None, *, L=None, b=None):
        from .. import _spawn
        if _spawn.active() is not None:
            # single-process front of the multi-GPU path: the posterior is built, sharded, by the worker processes
            return _spawn.condition(self, Y, X, L=L, b=b)
        from .. import config
        if config.matrix_free or (config.matrix_free_above and np.size(Y) > int(config.matrix_free_above)):
            from ._matrix_free import MatrixFreeConditionalGaussianProcess
            return MatrixFreeConditionalGaussianProcess.from_observations(self, Y, X, L=L, b=b)
        return ConditionalGaussianProcess.from_observations(self, Y, X, L=L, b=b)


# ---- joint draws (`RandomProcess.sample` of probnum, behind it `Normal.sample` / `cov_cholesky`) ------------------------
def _sample_size(size) -> tuple:
    if isinstance(size, (int, np.integer)):
        size = (int(size),)
    size = tuple(int(k) for k in size)
    if any(k < 0 for k in size):
        raise ValueError(f"`size` must not be negative, got {size}")
    return size


def _sample_damping(damping) -> float:
    from .. import config
    d = float(config.sample_damping if damping is None else damping)
    if not d >= 0.0:
        raise ValueError(f"`damping` must be a non-negative number, got {damping!r}")
    return d


def _sample_context():
    from .. import _spawn
    if _spawn.active() is not None:
        raise NotImplementedError("`sample` is not available through the `lp.spawn` multi-GPU front (single GPU only)")
    ctx = _engine.default_context()
    if ctx.distributed:
        raise NotImplementedError("`sample` is not available in a multi-GPU job (single GPU only)")
    return ctx


def _sample_points(gp, x):
    x = np.asarray(x, dtype=np.double)
    nd = gp.input_ndim
    if nd and (x.ndim < nd or x.shape[x.ndim - nd:] != tuple(gp.input_shape)):
        raise ValueError(f"The shape of the input {x.shape} is not compatible with the input shape {tuple(gp.input_shape)} of the process.")
    return gp._flat(x)


def _factor_damped(S: "_engine.GramMatrix", delta: float, damping: float) -> None:
    S.add_diag(0, None, delta)
    info = S.potrf()
    if info != 0:
        raise np.linalg.LinAlgError(
            f"{info}-th leading minor of the (padded) covariance at the sample points is not positive definite with damping = {damping:g} "
            f"(delta = {delta:g} on the diagonal); pass a larger `damping`")


def _cached_factor(gp, X, delta, coeffs_key):
    c = getattr(gp, "_sample_cache", None)
    if c is None or c[0] != (_engine.option_epoch(), delta, coeffs_key) or c[1].shape != X.shape or not np.array_equal(c[1], X):
        return None
    return c[2], c[3]


def _draws(S: "_engine.GramMatrix", mean: np.ndarray, z: np.ndarray, size: tuple, batch: tuple) -> np.ndarray:
    """draw[s] = mean + C z[s] for every z[s] of `z` (shape size + (M,)): one product on the device."""
    M = mean.size
    out = S.factor_matmul(np.ascontiguousarray(z.reshape(-1, M).T), mean)          # (M, number of draws)
    return np.ascontiguousarray(out.T).reshape(size + batch)


class _VariableCoeffs:
    """Canonical form of a functional built on a `diffops.VariableCoefficientOperator`, in the place of the coefficient map
    (`_preprocess_observations`): `weights[a, i] = f_a(x_i)`, evaluated on the host once per block, and the coefficient maps of
    the constant-coefficient parts `D_a`."""
    __slots__ = ("weights", "terms")

    def __init__(self, weights, terms):
        self.weights = np.ascontiguousarray(weights, dtype=np.double)
        self.terms = [dict(t) for t in terms]


_VARIABLE = "variable-coefficient operators (`VariableCoefficientOperator`)"


class _ObservationBlock:
    __slots__ = ("Y", "L", "b", "X", "coeffs", "points", "pred_mean", "vterms", "weights", "mixing", "mix", "rows")

    def __init__(self, Y, L, b, X, coeffs, points, pred_mean, mixing=None):
        self.Y, self.L, self.b, self.X = Y, L, b, X
        # observations through a matrix (`A @ L`): the rows of A as a stencil table over the points, (idx, w) on the host and
        # resident on the device; the block then has A's rows, not one row per point
        self.mixing, self.mix = mixing, None
        self.rows = points.n if mixing is None else int(mixing[0].shape[0])
        if mixing is not None:
            self.mix = _engine.Mix(points.ctx, mixing[0], mixing[1], points.n)
        self.vterms = self.weights = None
        if isinstance(coeffs, _VariableCoeffs):
            # L = sum_a f_a D_a: the coefficient maps of the D_a and the weights f_a(X), (A, n); no single coefficient map
            self.vterms, self.weights, coeffs = coeffs.terms, coeffs.weights, None
        self.coeffs = coeffs          # coefficient map of the functional's operator part
        self.points = points          # device point set
        self.pred_mean = pred_mean    # L[m] + b.mean, flattened


def _block_terms(ob):
    """(weights (A, n), [coefficient map of D_a]) of an observation block  sum_a f_a D_a;  a constant-coefficient block is ONE
    term of weight 1."""
    if ob.vterms is not None:
        return ob.weights, ob.vterms
    return np.ones((1, ob.points.n)), [ob.coeffs]


def _has_variable(blocks) -> bool:
    return any(ob.vterms is not None for ob in blocks)


_MIXED = "observations through a matrix (`A @ L`)"


def _has_mixed(blocks) -> bool:
    return any(ob.mix is not None for ob in blocks)


def _mix_apply(ob, Z: np.ndarray) -> np.ndarray:
    """A @ Z for the matrix of a mixed block, Z of shape (points, m); a plain block: Z."""
    if ob.mixing is None:
        return Z
    idx, w = ob.mixing
    return np.einsum("rs,rsm->rm", w, Z[idx])


def _mix_apply_transposed(ob, V: np.ndarray) -> np.ndarray:
    """A^T @ V for the matrix of a mixed block, V of shape (rows, m); a plain block: V."""
    if ob.mixing is None:
        return V
    idx, w = ob.mixing
    out = np.zeros((ob.points.n, V.shape[1]))
    np.add.at(out, idx, w[:, :, None] * V[:, None, :])
    return out


def _assemble_block(mat, base, bi, bj, row_block, col_block):
    """Block (bi, bj) of the Gram matrix, `col_block is row_block` for the diagonal block: the existing call for two
    constant-coefficient blocks, `lpgp_gram_assemble_weighted` (entry-wise from the flattened points, also for tensor grids: a
    weighted block is not a Kronecker product) as soon as either side has variable coefficients -- one pair (a, b) per pair
    of terms, weight 1 / A = 1 for a constant-coefficient side; `lpgp_gram_assemble_mixed` as soon as either side is a matrix
    block (`A @ L`), the other side's rows then its points."""
    sym = col_block is row_block
    if row_block.mix is not None or col_block.mix is not None:
        # the fused stencil kernel (`lpgp_gram_assemble_mixed`), a side without a table plain
        if row_block.vterms is not None or col_block.vterms is not None:
            raise NotImplementedError(f"{_MIXED} and {_VARIABLE} in one chain are not supported")
        mat.assemble_mixed(_lowered(base, row_block.coeffs, col_block.coeffs), row_block.points, row_block.mix,
                           None if sym else col_block.points, None if sym else col_block.mix, bi, bj)
        return
    if row_block.vterms is None and col_block.vterms is None:
        mat.assemble(_lowered(base, row_block.coeffs, col_block.coeffs), row_block.points, None if sym else col_block.points, bi, bj)
        return
    w0, t0 = _block_terms(row_block)
    w1, t1 = _block_terms(col_block)
    pairs = [(_lowered(base, ca, cb), a, b) for a, ca in enumerate(t0) for b, cb in enumerate(t1)]
    mat.assemble_weighted(pairs, w0, None if sym else w1, row_block.points, None if sym else col_block.points, bi, bj)


class _GramOperator:
    """What `ConditionalGaussianProcess.gram` returns (`_conditional.py:92-94`): the resident factorisation behind the part
    of probnum's `LinearOperator` protocol the reference's callers use (`solve`, `inv`, `cholesky`,
    `todense`, `@`, `.T`, `det` / `logabsdet`, `trace`).  The Gram matrix itself no longer exists in HBM (it was factored
    in place): products `G @ V` re-evaluate its blocks matrix-free (`lpgp_kernel_matvec`) and add the noise terms."""

    def __init__(self, cgp: "ConditionalGaussianProcess"):
        self._cgp = cgp

    @property
    def shape(self):
        n = sum(ob.rows for ob in self._cgp._blocks)
        return (n, n)

    dtype = np.dtype(np.double)
    is_symmetric = True
    is_positive_definite = True

    @property
    def T(self):
        return self

    def solve(self, B):
        self._cgp._check_current()
        return self._cgp._state.mat.potrs(B)

    def inv(self):
        return _GramInverse(self)

    def cholesky(self, lower: bool = True):
        self._cgp._check_current()
        Lf = self._cgp._state.mat.todense("factor")
        return Lf if lower else Lf.T

    def todense(self):
        Lf = self.cholesky(True)
        return _engine.gemm(self._cgp._state.ctx, Lf, Lf, transb=True)      # L L^T on the device (round 6; an O(n^3) NumPy product until then)

    def logabsdet(self) -> float:
        """log det G = 2 sum_i log L_ii from the diagonal of the resident factor (`lpgp_mat_factor_diag`)."""
        self._cgp._check_current()
        d = self._cgp._state.mat.factor_diag()
        return float(2.0 * np.sum(np.log(d)))

    def det(self) -> float:
        return float(np.exp(self.logabsdet()))

    def trace(self) -> float:
        """Sum of the diagonal of G: the differentiated kernel at coinciding points, block by block, plus the noise."""
        cgp = self._cgp
        base = cgp._prior.cov
        tr = 0.0
        for ob in cgp._blocks:
            if ob.mix is not None:
                raise NotImplementedError(f"`gram.trace()` is not available on a chain with {_MIXED}")
            if ob.vterms is not None:
                # sum_i sum_ab f_a(x_i) f_b(x_i) (D_a k D_b'^*)(x_i, x_i)
                for a, ca in enumerate(ob.vterms):
                    for b, cb in enumerate(ob.vterms):
                        tr += float(ob.weights[a] @ ob.weights[b]) * _engine.kernel_diag(cgp._state.ctx, _lowered(base, ca, cb))
                tr += float(np.sum(_noise_diag(ob)))
                continue
            k = covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(base), *_combine(base, ob.coeffs, ob.coeffs))
            tr += ob.rows * _engine.kernel_diag(cgp._state.ctx, k.lower())
            tr += float(np.sum(_noise_diag(ob)))
        return tr

    def __matmul__(self, V):
        cgp = self._cgp
        V = np.asarray(V, dtype=np.double)
        n = self.shape[0]
        if V.shape[0] != n or V.ndim > 2:
            raise ValueError(f"operand of shape {V.shape} does not match the Gram operator {self.shape}")
        V2 = V.reshape(n, -1)
        out = np.zeros_like(V2)
        base = cgp._prior.cov
        offs = np.cumsum([0] + [ob.rows for ob in cgp._blocks])
        for i, bi in enumerate(cgp._blocks):
            for j, bj in enumerate(cgp._blocks):
                if bi.rows == 0 or bj.rows == 0:
                    continue
                if bi.mix is not None or bj.mix is not None:
                    # A_i K(X_i, X_j) (A_j^T V): the mixing on the host, the product with K matrix-free on the points
                    if bi.vterms is not None or bj.vterms is not None:
                        raise NotImplementedError(f"{_MIXED} and {_VARIABLE} in one chain are not supported")
                    k = covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(base), *_combine(base, bi.coeffs, bj.coeffs))
                    KV = _engine.kernel_matvec(cgp._state.ctx, k.lower(), bi.points, bj.points,
                                               np.ascontiguousarray(_mix_apply_transposed(bj, V2[offs[j]:offs[j + 1]])))
                    out[offs[i]:offs[i + 1]] += _mix_apply(bi, KV)
                    continue
                if bi.vterms is not None or bj.vterms is not None:
                    # diag(f_a) K_ab diag(g_b) V, pair by pair, the scalings on the host
                    (w0, t0), (w1, t1) = _block_terms(bi), _block_terms(bj)
                    Vj = V2[offs[j]:offs[j + 1]]
                    for a, ca in enumerate(t0):
                        for b, cb in enumerate(t1):
                            out[offs[i]:offs[i + 1]] += w0[a][:, None] * _engine.kernel_matvec(
                                cgp._state.ctx, _lowered(base, ca, cb), bi.points, bj.points, np.ascontiguousarray(w1[b][:, None] * Vj))
                    continue
                k = covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(base), *_combine(base, bi.coeffs, bj.coeffs))
                out[offs[i]:offs[i + 1]] += _engine.kernel_matvec(cgp._state.ctx, k.lower(), bi.points, bj.points,
                                                                  np.ascontiguousarray(V2[offs[j]:offs[j + 1]]))
            if bi.b is not None and isinstance(bi.b, randvars.Normal):
                if bi.b.cov_diag is not None:
                    out[offs[i]:offs[i + 1]] += np.asarray(bi.b.cov_diag)[:, None] * V2[offs[i]:offs[i + 1]]
                else:
                    out[offs[i]:offs[i + 1]] += np.asarray(bi.b.cov).reshape(bi.rows, bi.rows) @ V2[offs[i]:offs[i + 1]]
        return out.reshape(V.shape)


def _noise_diag(ob) -> np.ndarray:
    if ob.b is None or not isinstance(ob.b, randvars.Normal):
        return np.zeros(0)
    if ob.b.cov_diag is not None:
        return np.asarray(ob.b.cov_diag, dtype=np.double)
    return np.diag(np.asarray(ob.b.cov).reshape(ob.rows, ob.rows))


class _GramInverse:
    """`gram.inv()`: products are solves with the resident factor."""

    def __init__(self, gram: _GramOperator):
        self._gram = gram

    @property
    def shape(self):
        return self._gram.shape

    @property
    def T(self):
        return self

    def __matmul__(self, B):
        return self._gram.solve(B)

    def inv(self):
        return self._gram

    def todense(self):
        return self._gram.solve(np.eye(self.shape[0]))

    def diagonal(self) -> np.ndarray:
        """diag(G^{-1}) from the resident factor (`lpgp_mat_inverse_diag`): neither the identity nor the inverse visits the host."""
        cgp = self._gram._cgp
        if not cgp._blocks:
            return np.zeros(0)
        _evidence_context("gram.inv().diagonal")
        cgp._check_current()
        return cgp._state.mat.inverse_diag()


class _DeviceState:
    """Device-resident state shared along a chain of conditionings: ONE matrix whose leading
    blocks are the factor of every earlier posterior of the chain (a block append never touches the
    leading part of the factor).  A posterior object uses the leading `len(blocks)` blocks through a
    view (`lpgp_mat_set_view`), so earlier objects of the chain stay usable; conditioning an object
    that has already been extended (branching) continues on a copy of its part of the factor."""

    def __init__(self, ctx, mat=None, blocks=(), capacity_hint=0):
        from .. import config

        self.ctx = ctx
        self.mat = mat if mat is not None else _engine.GramMatrix(ctx, capacity_hint=config.gram_capacity_hint or capacity_hint)
        self.view = None             # number of blocks the device-resident weights / residual belong to
        self.weights_key = None
        self.residual_key = None
        self.blocks = list(blocks)   # the observation blocks in the matrix, in order (identity decides whether an object is alive)
        self.pending = False         # factorisations enqueued (or deferred) whose status has not been read (config.lazy_factorization)
        self.deferred = False        # the newest block is assembled but its factorisation not even enqueued: whoever needs the
                                     # factor first enqueues it (`flush`) -- or `predict`, which rides inside it (`lpgp_potrf_predict`)
        self.deferred_rows = 0       # rows of the blocks that are assembled but not factored
        self.failure = None          # message of the last failure found by `verify`

    def flush(self) -> None:
        """Enqueue the factorisation of a block that was only assembled so far."""
        if self.deferred:
            self.deferred = False
            self.deferred_rows = 0
            self.mat.potrf_enqueue()

    def invalidate(self) -> None:
        """The device dropped the resident representer weights / residual (`lpgp_mat_add_block`, `lpgp_mat_pop_block`
        and a growing matrix all clear them): forget which object they belonged to."""
        self.view = None
        self.weights_key = None
        self.residual_key = None

    def verify(self) -> None:
        """Read the status of the enqueued factorisations (one host synchronisation, at the first use of the factor).
        A block that was not positive definite is dropped together with everything appended after it -- the leading
        part of the factor is untouched by an append -- and the objects that own those blocks raise from now on."""
        self.flush()
        if not self.pending:
            return
        self.pending = False
        try:
            info, block = self.mat.check()
        except _engine._lib.LpgpError as exc:
            # not a pivot: a hand-over inside a resident kernel timed out and the factor is undefined (the library keeps the
            # matrix marked so, every later call on it fails).  EVERY object of the chain is dead from here on -- ADVICE r5: the
            # error used to be raised once, and the next `predict` ran on the garbage factor as if it had been verified
            self.failure = str(exc)
            del self.blocks[:]
            self.invalidate()
            raise
        if info == 0:
            return
        self.failure = f"{info}-th leading minor of the (padded) Gram matrix is not positive definite"
        self.mat.set_view(-1)
        self.mat.truncate(block)
        del self.blocks[block:]
        self.invalidate()

    def owns(self, blocks) -> bool:
        """Are `blocks` (an object's) still the leading blocks of this matrix?"""
        n = len(blocks)
        return n <= len(self.blocks) and (n == 0 or self.blocks[n - 1] is blocks[n - 1])

    def use(self, nblocks: int) -> None:
        """Make the leading `nblocks` blocks the matrix every following call sees."""
        if nblocks == 0:
            return
        if self.mat.num_blocks != nblocks:
            self.flush()             # (a view is a statement about the FACTOR: nothing stays merely assembled behind it)
            self.mat.set_view(nblocks)
        if self.view != nblocks:
            self.view = nblocks
            self.weights_key = None
            self.residual_key = None


def _evidence_context(what: str):
    from .. import _spawn
    if _spawn.active() is not None:
        raise NotImplementedError(f"`{what}` is not available through the `lp.spawn` multi-GPU front (single GPU only)")
    ctx = _engine.default_context()
    if ctx.distributed:
        raise NotImplementedError(f"`{what}` is not available in a multi-GPU job (single GPU only)")
    return ctx


class LeaveOneOut:
    """Result of `ConditionalGaussianProcess.leave_one_out()`: per observation, in Gram order (conditioning order, each block
    flattened in C order), the predictive distribution of the NOISY observation y_i given all the others -- `mean`, `var`
    (the observation's own `b` variance included), `std` -- its log density at the observed value, `log_predictive_density`,
    and `total`, the sum of the densities (the leave-one-out pseudo-likelihood)."""

    __slots__ = ("mean", "var", "log_predictive_density", "total")

    def __init__(self, mean, var, log_predictive_density, total):
        self.mean, self.var, self.log_predictive_density, self.total = mean, var, log_predictive_density, float(total)

    @property
    def std(self) -> np.ndarray:
        return np.sqrt(np.maximum(self.var, 0.0))

    def __repr__(self):
        return f"LeaveOneOut(n={self.mean.size}, total={self.total:.6g})"


def _normalise_folds(folds, block_sizes):
    """(fold_of, folds) of `ConditionalGaussianProcess.cross_validate`: `fold_of[i]` = the fold of row i in Gram order (int32, -1: in
    no fold) and the folds as a tuple of sorted int64 index arrays.  `folds`: "blocks" (one fold per observation block), an int k
    with 2 <= k <= n (row i goes to fold i % k), or a sequence of 1-D integer arrays, disjoint, each non-empty; they need not cover
    all rows.  `block_sizes`: the rows of the observation blocks.  Needs no device.  `ValueError` on anything else."""
    sizes = [int(b) for b in block_sizes]
    n = sum(sizes)
    if isinstance(folds, str):
        if folds != "blocks":
            raise ValueError(f'`folds` must be "blocks", an int or a sequence of index arrays, got {folds!r}')
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        return (np.repeat(np.arange(len(sizes), dtype=np.int32), sizes),
                tuple(np.arange(offs[b], offs[b + 1], dtype=np.int64) for b in range(len(sizes))))
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, (bool, np.bool_)):
        k = int(folds)
        if not 2 <= k <= n:
            raise ValueError(f"a number of strided folds must lie in 2 .. {n} (the number of observations), got {k}")
        rows = np.arange(n, dtype=np.int64)
        if k == n:
            return rows.astype(np.int32), tuple(rows.reshape(n, 1))
        return (rows % k).astype(np.int32), tuple(rows[f::k] for f in range(k))
    else:
        try:
            raw = [np.asarray(f) for f in folds]
        except TypeError:
            raise ValueError(f'`folds` must be "blocks", an int or a sequence of index arrays, got {folds!r}') from None
        lists = []
        for f, a in enumerate(raw):
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"fold {f} must be a 1-D array of integer row indices, got shape {a.shape} and dtype {a.dtype}")
            lists.append(a.astype(np.int64))
    if not lists:
        raise ValueError("no folds")
    fold_of = np.full(n, -1, dtype=np.int32)
    out = []
    for f, idx in enumerate(lists):
        if idx.size == 0:
            raise ValueError(f"fold {f} is empty")
        if idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"fold {f} has a row index outside 0 .. {n - 1}")
        idx = np.sort(idx)
        if np.any(idx[1:] == idx[:-1]) or np.any(fold_of[idx] >= 0):
            raise ValueError(f"fold {f} overlaps an earlier fold or names a row twice: the folds must be disjoint")
        fold_of[idx] = f
        out.append(idx)
    return fold_of, tuple(out)


class FoldPredictions:
    """Result of `ConditionalGaussianProcess.cross_validate()`: `folds`, the row indices (Gram order, sorted) of every fold; per
    observation the predictive distribution of the NOISY observation given all observations OUTSIDE its fold -- `mean`, `var`
    (the observation's own `b` variance included), `std`, NaN for a row in no fold; per fold the joint log density of its
    observations at the observed values, `log_predictive_density`, and `total`, their sum in fold order; `cov`, the joint (b, b)
    predictive covariance of every fold (rows as in `folds`), or None if it was not asked for."""

    __slots__ = ("folds", "mean", "var", "log_predictive_density", "total", "cov")

    def __init__(self, folds, mean, var, log_predictive_density, total, cov=None):
        self.folds, self.mean, self.var, self.log_predictive_density, self.total, self.cov = folds, mean, var, log_predictive_density, float(total), cov

    @property
    def std(self) -> np.ndarray:
        return np.sqrt(np.maximum(self.var, 0.0))

    def __repr__(self):
        return f"FoldPredictions(n={self.mean.size}, folds={len(self.folds)}, total={self.total:.6g})"


class EvidenceGradient:
    """Result of `ConditionalGaussianProcess.log_marginal_likelihood_gradient()`: `value`, the log marginal likelihood itself, and
    its derivatives with respect to the LOGARITHMS of the hyperparameters (every entry 1/2 w^T dG w - 1/2 tr(G^{-1} dG), GPML eq. 5.9):
    `log_output_scale` (G,), by the variance scale of summand g of the prior covariance (its factor in front of the product of
    univariate kernels); `log_lengthscales` (G, d), by lengthscale j of summand g; `log_noise` (B,), by a factor tau_b in front of
    the noise covariance `b.cov` of observation block b, at tau_b = 1 (0.0 for a block without noise).  G summands, d input
    dimensions, B observation blocks in conditioning order."""

    __slots__ = ("value", "log_output_scale", "log_lengthscales", "log_noise")

    def __init__(self, value, log_output_scale, log_lengthscales, log_noise):
        self.value = float(value)
        self.log_output_scale, self.log_lengthscales, self.log_noise = log_output_scale, log_lengthscales, log_noise

    def __repr__(self):
        return (f"EvidenceGradient(value={self.value:.6g}, summands={self.log_output_scale.size}, "
                f"dims={self.log_lengthscales.shape[1]}, blocks={self.log_noise.size})")


def _block_noise(ob):
    """(scalar, diag, dense) of the noise covariance of an observation block, as `_extend` hands it to the library."""
    n = ob.rows
    scalar, diag, dense = 0.0, None, None
    if ob.b is not None and isinstance(ob.b, randvars.Normal):
        if ob.b.cov_diag is not None:
            diag = np.ascontiguousarray(ob.b.cov_diag, dtype=np.double)
        else:
            cov = np.asarray(ob.b.cov).reshape(n, n)
            if np.any(cov - np.diag(np.diag(cov)) != 0.0):
                dense = np.ascontiguousarray(cov, dtype=np.double)
            else:
                diag = np.ascontiguousarray(np.diag(cov), dtype=np.double)
        if diag is not None and diag.size and np.all(diag == diag.flat[0]):
            scalar, diag = float(diag.flat[0]), None
    return scalar, diag, dense


def _refuse_variable_off_path(coeffs, ctx=None) -> None:
    """Variable-coefficient observations exist on the dense single-GPU path only: refuse a multi-GPU context before any
    device work (the `lp.spawn` front and the matrix-free posteriors refuse on their own)."""
    if isinstance(coeffs, _VariableCoeffs) and (ctx if ctx is not None else _engine.default_context()).distributed:
        raise NotImplementedError(f"{_VARIABLE} are not supported in a multi-GPU job (single GPU only)")


def _refuse_mixed_off_path(L, ctx=None):
    """`L.mixing()`, after refusing a mixed block in a multi-GPU context before any device work (see `_refuse_variable_off_path`)."""
    mixing = L.mixing()
    if mixing is not None and (ctx if ctx is not None else _engine.default_context()).distributed:
        raise NotImplementedError(f"{_MIXED} are not supported in a multi-GPU job (single GPU only)")
    return mixing


_ROWS_SEEN_MAX = 4096        # (a hint only, and only where re-allocation matters: 128 MB; beyond, a copy is noise against the O(n^3) work)


class ConditionalGaussianProcess(GaussianProcess):
    @classmethod
    def from_observations(cls, prior: GaussianProcess, Y, X=None, *, L=None, b=None):
        Yf, Lf, bf, Xpts, coeffs, pred_mean = cls._preprocess_observations(prior=prior, Y=Y, X=X, L=L, b=b)
        # (room for the longest chain this prior has been conditioned into so far: the same model is typically conditioned again
        #  and again -- new data, new hyperparameters' worth of right-hand sides -- and a matrix that outgrows its allocation in the
        #  middle of a chain is re-allocated and copied: eight launches of a 1 152-row problem's sixty)
        _refuse_variable_off_path(coeffs)
        mixing = _refuse_mixed_off_path(Lf)
        state = _DeviceState(_engine.default_context(), capacity_hint=getattr(prior, "_rows_seen", 0))
        block = _ObservationBlock(Yf, Lf, bf, Xpts, coeffs, Lf.device_points(state.ctx), pred_mean, mixing)
        return cls._extend(prior, state, (), block)

    @classmethod
    def _extend(cls, prior, state, old_blocks, new_block):
        """Append `new_block` to the chain `old_blocks` of `state` and return the new posterior.

        A chain that contains a block with VARIABLE coefficients (`diffops.VariableCoefficientOperator`) -- the new block or
        an earlier one -- takes the eager separate-call path whatever `config.lazy_factorization` says: factorisations still
        deferred are flushed and verified first, then `lpgp_mat_add_block`, one `lpgp_gram_assemble_weighted` per block of
        the row where either side is variable (the existing assembly otherwise), the noise, `lpgp_potrf`; a Gram matrix
        that is not positive definite pops the block and raises exactly as the one-call path does.  A chain with a matrix
        block (`A @ L`, `lpgp_gram_assemble_mixed`) goes the same way."""
        from .. import config

        if new_block.rows == 0:
            # no observations: nothing to assemble or factor, the factor in HBM stays as it is (and
            # stays valid for the object this one was derived from)
            return cls(prior=prior, blocks=tuple(old_blocks), state=state, representer_weights=None)
        lazy = bool(config.lazy_factorization) and not state.ctx.distributed      # (a context that joined a job -- even of one rank -- factors collectively)
        if not state.owns(old_blocks):
            # the object being conditioned rests on a block that was not positive definite and has been dropped:
            # `state.blocks` only ever shrinks through `verify`'s truncation, so not owning its blocks means dead whether
            # or not another factorisation is pending (with the check skipped while pending, a dead child's
            # rows were lowered against ITS points and appended onto the blocks of a sibling)
            raise np.linalg.LinAlgError(state.failure or "the Gram matrix of this posterior is not positive definite")
        if len(state.blocks) != len(old_blocks):
            # the object being conditioned has already been extended by another conditioning: this one
            # branches off on its own copy of the leading part of the factor (multi-GPU: not supported)
            state.verify()
            if not state.owns(old_blocks):
                raise np.linalg.LinAlgError(state.failure)
            if len(state.blocks) != len(old_blocks):
                state = _DeviceState(state.ctx, state.mat.clone(len(old_blocks)), old_blocks)
        mixed = new_block.mix is not None or _has_mixed(old_blocks)
        variable = new_block.vterms is not None or _has_variable(old_blocks) or mixed      # (a chain with a matrix block goes the same way)
        if variable:
            if state.ctx.distributed:
                raise NotImplementedError(f"{_MIXED if mixed else _VARIABLE} are not supported in a multi-GPU job (single GPU only)")
            state.verify()
            if not state.owns(old_blocks):
                raise np.linalg.LinAlgError(state.failure or "the Gram matrix of this posterior is not positive definite")
        state.use(len(old_blocks))
        if variable:
            return cls._extend_eager(prior, state, old_blocks, new_block)
        # lazy: a LARGE block that an earlier conditioning only assembled STAYS deferred when further blocks follow -- they are
        # factored together at the first use, with the prediction riding inside all of it (c5: the 32 768-row collocation block
        # is followed by a small block of interior values: 297 -> 290 ms).  Small deferred blocks are factored now: their tiny
        # kernels run while the host prepares the next conditioning (deferring them all costs small problems 10 %: the device
        # would idle through the chain's host time and do everything at the end).
        if state.deferred and (not lazy or state.deferred_rows < int(config.defer_min_rows)):
            state.flush()
        mat = state.mat
        base = prior.cov
        state.invalidate()           # the device drops the resident weights / residual with the new block (also when it is rolled back)
        # ONE call through the binding per conditioning (`lpgp_mat_condition`): the block row of the Gram matrix --
        # lower-left blocks (L_new k L_j'^*)(X_new, X_j) (`_conditional.py:270`), diagonal block --, the measurement noise
        # gram + b.cov (`_conditional.py:392-394`) and the factorisation.  A failed conditioning leaves the object it was
        # called on intact, as in the reference: the library drops the new block again, the leading factor is never touched.
        row = [(_lowered(base, new_block.coeffs, ob.coeffs), ob.points) for ob in old_blocks]
        row.append((_lowered(base, new_block.coeffs, new_block.coeffs), None))
        n = new_block.rows
        scalar, diag, dense = 0.0, None, None
        if new_block.b is not None and isinstance(new_block.b, randvars.Normal):
            if new_block.b.cov_diag is not None:
                diag = np.ascontiguousarray(new_block.b.cov_diag, dtype=np.double)
            else:
                cov = np.asarray(new_block.b.cov).reshape(n, n)
                if np.any(cov - np.diag(np.diag(cov)) != 0.0):
                    dense = cov
                else:
                    diag = np.ascontiguousarray(np.diag(cov), dtype=np.double)
            if diag is not None and diag.size and np.all(diag == diag.flat[0]):
                scalar, diag = float(diag.flat[0]), None          # sigma^2 I: nothing to upload
        # lazy: the block is assembled and its factorisation DEFERRED to the first call that needs the factor (the next
        # conditioning, `mean`, `cov`, `representer_weights`, ... enqueue it; a `predict` rides inside it)
        info = mat.condition(n, new_block.points, row, noise_scalar=scalar, noise_diag=diag, noise_dense=dense, lazy=2 if lazy else 0)
        if info != 0:
            raise np.linalg.LinAlgError(
                f"{info}-th leading minor of the (padded) Gram matrix is not positive definite")
        state.blocks.append(new_block)
        rows = sum(-(-k // 128) * 128 for k in mat.block_sizes)
        if getattr(prior, "_rows_seen", 0) < rows <= _ROWS_SEEN_MAX:
            prior._rows_seen = rows
        state.pending = state.pending or lazy
        state.deferred_rows = (state.deferred_rows if state.deferred else 0) + n if lazy else 0
        state.deferred = lazy
        blocks = tuple(old_blocks) + (new_block,)
        # the representer weights are solved on first use (`representer_weights`, `mean`, ...):
        # in a chain of conditionings only the last object's weights are ever needed
        return cls(prior=prior, blocks=blocks, state=state, representer_weights=None)

    @classmethod
    def _extend_eager(cls, prior, state, old_blocks, new_block):
        """The separate-call conditioning of a chain with a variable-coefficient block (see `_extend`)."""
        mat, base = state.mat, prior.cov
        state.invalidate()
        scalar, diag, dense = _block_noise(new_block)
        bi = mat.add_block(new_block.rows)
        try:
            for j, ob in enumerate(tuple(old_blocks) + (new_block,)):
                _assemble_block(mat, base, bi, j, new_block, ob)
            if dense is not None:
                mat.add_dense(bi, dense)
            elif diag is not None or scalar != 0.0:
                mat.add_diag(bi, diag, scalar)
            info = mat.potrf()
        except BaseException:
            mat.pop_block()
            raise
        if info != 0:
            mat.pop_block()
            raise np.linalg.LinAlgError(
                f"{info}-th leading minor of the (padded) Gram matrix is not positive definite")
        state.blocks.append(new_block)
        rows = sum(-(-k // 128) * 128 for k in mat.block_sizes)
        if getattr(prior, "_rows_seen", 0) < rows <= _ROWS_SEEN_MAX:
            prior._rows_seen = rows          # (the capacity hint of the next chain from this prior, as in `_extend`)
        return cls(prior=prior, blocks=tuple(old_blocks) + (new_block,), state=state, representer_weights=None)

    def __init__(self, *, prior, blocks, state, representer_weights, test_coeffs=None):
        self._prior = prior
        self._blocks = tuple(blocks)
        self._state = state
        self._representer_weights = representer_weights
        d = max(int(np.prod(prior.input_shape, dtype=int)), 1)
        self._test_coeffs = dict(test_coeffs) if test_coeffs is not None else {(0,) * d: 1.0}
        # `mean` / `cov` are built on access (below): storing them here would make every
        # posterior part of a reference cycle (posterior -> mean -> posterior), and the
        # multi-GB device matrix of a dropped posterior would then live until the cyclic
        # collector happens to run (measured at c4: a fresh 35 GB hipMalloc per step, +1 s)
        self._mean = None
        self._cov = None
        self._pred_cache = None      # (option epoch, points, mean, var or None) of the last prediction: a posterior is an immutable
                                     # value, so `u.mean(x)` followed by `u.std(x)` (notebook 0001 cell 22) shares one pass

    @property
    def mean(self):
        return _PosteriorMean(self)

    @property
    def cov(self):
        return _PosteriorCovarianceFunction(self)

    @property
    def input_shape(self):
        return self._prior.input_shape

    @property
    def input_ndim(self):
        return len(self._prior.input_shape)

    # -- reference attribute surface --
    @property
    def gram(self):
        return _GramOperator(self)

    @property
    def representer_weights(self) -> np.ndarray:
        """G^{-1}(Y - L[m] - b.mean)  (`_conditional.py:96-110`: computed lazily there too)."""
        self._ensure_weights()
        return self._representer_weights

    def _residual(self) -> np.ndarray:
        if not self._blocks:
            return np.zeros(0)
        return np.concatenate([ob.Y - ob.pred_mean for ob in self._blocks])

    def _ensure_weights(self):
        if not self._blocks:
            self._representer_weights = np.zeros(0)
            return
        self._check_current()
        if self._representer_weights is None or self._state.weights_key != len(self._blocks):
            # (second case: the device copy of the weights belongs to another view of the same factor)
            self._representer_weights = self._state.mat.solve_weights(self._residual())
            self._state.weights_key = len(self._blocks)

    def _ensure_residual(self):
        """Mean AND variance need no weights: `K_xX G^{-1} r = V^T (L^{-1} r)` with the solved
        cross-covariance `V = L^{-1} K_Xx` the variance computes anyway; the library only needs
        the residual (its forward substitution hides under the solve for `V`)."""
        if not (self._state.pending and self._state.owns(self._blocks) and self._state.view == len(self._blocks)):
            self._check_current()        # (not from a speculative `predict`: see `_use_unverified`)
        if self._state.residual_key != len(self._blocks):
            self._state.mat.set_residual(self._residual())
            self._state.residual_key = len(self._blocks)

    @property
    def prior(self):
        return self._prior

    def _check_current(self):
        """Point the shared device matrix at THIS object's blocks.  A later `condition_on_observations`
        appended to the same matrix without touching its leading part, so an earlier posterior keeps
        working (the reference's posteriors are immutable values).  First use of the factor: the status of the
        factorisations enqueued so far is read here (`config.lazy_factorization = True`; by default every conditioning has
        read its own), and an object whose own block -- or a block it was conditioned on -- was not positive definite
        raises."""
        self._state.verify()
        if not self._state.owns(self._blocks):
            raise np.linalg.LinAlgError(self._state.failure or "the Gram matrix of this posterior is not positive definite")
        self._state.use(len(self._blocks))

    def _use_unverified(self) -> bool:
        """`predict` with factorisations still in flight: enqueue the whole prediction behind them FIRST and read their
        status afterwards (`_verify_after`) -- the device then goes from the last panel of the factorisation straight into
        the cross-covariance and the forward substitution, with no host round trip in between.  A factor that turns out not
        to be positive definite costs a prediction computed on garbage, which is discarded.  False: nothing is pending (or
        this object is already known to be dead): the ordinary order applies."""
        st = self._state
        if not st.pending or not st.owns(self._blocks):
            return False
        st.use(len(self._blocks))
        return True

    def _verify_after(self):
        self._state.verify()
        if not self._state.owns(self._blocks):
            raise np.linalg.LinAlgError(self._state.failure or "the Gram matrix of this posterior is not positive definite")

    def condition_on_observations(self, Y, X=None, *, L=None, b=None):
        if any(v != 1.0 or any(mi) for mi, v in self._test_coeffs.items()):
            raise NotImplementedError("conditioning a transformed posterior is not supported")
        Yf, Lf, bf, Xpts, coeffs, pred_mean = self._preprocess_observations(
            prior=self._prior, Y=Y, X=X, L=L, b=b)
        _refuse_variable_off_path(coeffs, self._state.ctx)
        mixing = _refuse_mixed_off_path(Lf, self._state.ctx)
        block = _ObservationBlock(Yf, Lf, bf, Xpts, coeffs, Lf.device_points(self._state.ctx), pred_mean, mixing)
        from .. import config
        if config.matrix_free_above and not self._state.ctx.distributed and \
                sum(ob.rows for ob in self._blocks) + block.rows > int(config.matrix_free_above):
            if block.mix is not None or _has_mixed(self._blocks):
                raise NotImplementedError(f"{_MIXED} are not supported on matrix-free posteriors (this chain has outgrown "
                                          "`config.matrix_free_above`)")
            if block.vterms is not None or _has_variable(self._blocks):
                raise NotImplementedError(f"{_VARIABLE} are not supported on matrix-free posteriors (this chain has outgrown "
                                          "`config.matrix_free_above`)")
            # (the threshold used to be consulted at the FIRST conditioning only -- a dense posterior re-conditioned past it
            #  stayed dense and could run out of memory.)  The chain continues matrix-free on the same observation blocks; the weights
            #  of this posterior, if they exist, warm-start the solve.
            from ._matrix_free import MatrixFreeConditionalGaussianProcess
            warm = None
            if self._representer_weights is not None:
                warm = np.concatenate([np.asarray(self._representer_weights, dtype=np.double), np.zeros(block.rows)])
            return MatrixFreeConditionalGaussianProcess(self._prior, self._blocks + (block,), warm_start=warm)
        return ConditionalGaussianProcess._extend(self._prior, self._state, self._blocks, block)

    @classmethod
    def _preprocess_observations(cls, *, prior, Y, X, L, b):
        # build measurement functional `L`
        if isinstance(L, LinearFunctional):
            if X is not None:
                raise TypeError("If `L` is a `LinearFunctional`, `X` must be `None`.")
        elif isinstance(L, LinearFunctionOperator):
            if X is None:
                raise ValueError("`X` must not be omitted if `L` is a `LinearFunctionOperator`.")
            L = L.to_linfunctl(X)
        elif L is None:
            if X is None:
                raise ValueError("`X` and `L` can not be omitted at the same time.")
            L = linfunctls._EvaluationFunctional(
                input_domain_shape=prior.input_shape, input_codomain_shape=prior.output_shape, X=X)
        else:
            raise TypeError("`L` must be a `LinearFunctional`, a `LinearFunctionOperator` or None")
        if L.input_domain_shape != tuple(prior.input_shape):
            raise ValueError(
                f"`L` acts on functions with input shape {L.input_domain_shape}, the prior has "
                f"input shape {prior.input_shape}")
        # measurement noise model
        if b is not None:
            b = randvars.asrandvar(b)
            if not isinstance(b, (randvars.Constant, randvars.Normal)):
                raise TypeError(f"`b` must be a `Normal` or a `Constant` `RandomVariable` ({type(b)=})")
            if tuple(b.shape) != tuple(L.output_shape):
                raise ValueError(f"{b.shape=} must be equal to {L.output_shape}")
        vt = L.variable_terms()
        Xpts = L.points()
        coeffs = L.coefficients_dict() if vt is None else _VariableCoeffs(*vt)
        # predictive mean  L[m] (+ b.mean)
        pred_mean = np.asarray(L(prior.mean), dtype=np.double).reshape(-1, order="C")
        Y = np.asarray(Y, dtype=np.double)
        if Y.shape != tuple(L.output_shape):
            raise ValueError(f"Expected Y to have shape {L.output_shape}, got shape {Y.shape}.")
        Y = Y.reshape(-1, order="C")
        if b is not None:
            pred_mean = pred_mean + np.asarray(b.mean, dtype=np.double).reshape(-1, order="C")
        return Y, L, b, Xpts, coeffs, pred_mean

    # -- prediction -----------------------------------------------------------------------
    def _cross(self, Xtest_pts):
        """K_Xx on the device: rows = all observation blocks, columns = test points."""
        st = self._state
        rhs = _engine.Rhs(st.ctx, st.mat, Xtest_pts.n)
        base = self._prior.cov
        if _has_variable(self._blocks) or _has_mixed(self._blocks):
            # block by block: sum_a diag(f_a(X_obs)) (D_a k Ltest'^*)(X_obs, x) for a variable-coefficient block
            # (`lpgp_cross_assemble_weighted`), A (L k Ltest'^*)(X_obs, x) by the stencil kernel for a matrix block
            # (`lpgp_cross_assemble_mixed`), the plain call for the others
            for bi, ob in enumerate(self._blocks):
                if ob.mix is not None:
                    rhs.cross_assemble_mixed(_lowered(base, ob.coeffs, self._test_coeffs), ob.points, ob.mix, Xtest_pts, bi)
                elif ob.vterms is None:
                    rhs.cross_assemble(_lowered(base, ob.coeffs, self._test_coeffs), ob.points, Xtest_pts, bi)
                else:
                    rhs.cross_assemble_weighted([(_lowered(base, c, self._test_coeffs), a, 0) for a, c in enumerate(ob.vterms)],
                                                ob.weights, ob.points, Xtest_pts, bi)
            return rhs
        # (L_obs k Ltest'^*)(X_obs, x)  == (Ltest k L_obs'^*)(x, X_obs) for the symmetric priors here; one call for the whole row
        # (blocks that share a descriptor share a launch)
        rhs.cross_assemble_row([(_lowered(base, ob.coeffs, self._test_coeffs), ob.points) for ob in self._blocks], Xtest_pts)
        return rhs

    def _prior_diag(self) -> float:
        base = self._prior.cov
        return _engine.kernel_diag(self._state.ctx, _lowered(base, self._test_coeffs, self._test_coeffs))

    def _prior_mean_at(self, x, n):
        m = self._prior.mean
        d = len(next(iter(self._test_coeffs)))
        c0 = self._test_coeffs.get((0,) * d, 0.0)
        if isinstance(m, functions.Constant):
            return np.full(n, c0 * float(m.value))
        # derivative read-outs of a non-constant mean: closed-form derivatives or NotImplementedError (functions.differentiate)
        return np.asarray(functions.apply_coefficients(self._test_coeffs, m)(x), dtype=np.double).reshape(-1)

    def predict(self, x, *, return_var: bool = True):
        """Posterior mean and marginal variance at `x` in one pass over the factor.

        In a multi-GPU job the prediction points are sharded over the ranks (contiguous slices): every rank
        solves for its own columns of the cross-covariance while the sharded factor is streamed past it panel by
        panel (`trsm_lower_dist`), and the results are gathered over the control plane; every rank returns the
        full arrays.  Collective: every rank calls it with the same `x`."""
        X, batch = self._flat(x)
        hit = self._cached_prediction(x, X, return_var)
        if hit is not None:
            return (hit[0].reshape(batch).copy(), hit[1].reshape(batch).copy()) if return_var else hit[0].reshape(batch).copy()
        speculative = self._use_unverified()
        if not speculative:
            self._check_current()
        ctx = self._state.ctx
        if X.shape[0] == 0 or not self._blocks:
            if speculative:
                self._verify_after()
            # nothing to predict, or nothing observed yet: the prior (`x1 is None` diagonal)
            mean = self._prior_mean_at(X if self.input_ndim else X[:, 0], X.shape[0]).reshape(batch)
            if not return_var:
                return mean
            return mean, np.full(batch, self._prior_diag() if X.shape[0] else 0.0)
        if ctx.world > 1 and X.shape[0] >= ctx.world:
            bounds = np.linspace(0, X.shape[0], ctx.world + 1).astype(int)
            lo, hi = bounds[ctx.rank], bounds[ctx.rank + 1]
            m_loc, v_loc = self._predict_local(None, X[lo:hi], return_var)
            parts = ctx.comm.allgather((m_loc, v_loc))
            mean = np.concatenate([p[0] for p in parts]).reshape(batch)
            if not return_var:
                return mean
            return mean, np.concatenate([p[1] for p in parts]).reshape(batch)
        from .. import config
        # `config.variance_with_mean`: a mean-only request computes the variance in the same pass and keeps it for the `std(x)`
        # that usually follows (either mode; in lazy mode that pass is the fused factor-and-predict pipeline)
        mean, var = self._predict_local(x, X, return_var or bool(config.variance_with_mean), speculative)
        if speculative:
            self._verify_after()
        self._pred_cache = (_engine.option_epoch(), X.copy(), mean.copy(), None if var is None else var.copy())
        mean = mean.reshape(batch)
        if not return_var:
            return mean
        return mean, var.reshape(batch)

    def _cached_prediction(self, x, X, need_var):
        c = self._pred_cache
        if c is None or (need_var and c[3] is None):
            return None
        # same points BY VALUE (the caller may have changed its array in place), same tuning options of the library
        if c[0] != _engine.option_epoch() or c[1].shape != X.shape or not np.array_equal(c[1], X):
            return None
        return c[2], c[3]

    def _predict_local(self, x_original, X, return_var, speculative=False):
        # the cross-covariance launches first: the device assembles it while the host stages the residual (a 135-KB upload
        # at c3, on the copy stream) or the weights are solved for
        if not speculative:
            self._check_current()
        from .. import config

        st = self._state
        pts = _engine.as_points(st.ctx, x_original, X)
        # A factorisation that is still deferred (lazy mode, this object's own block): the prediction rides INSIDE it
        # (`lpgp_potrf_predict`) -- for mean and variance together (a mean-only request arrives here as one if
        # `config.variance_with_mean` is set); a plain mean-only request enqueues the factorisation and solves for the weights
        fuse = speculative and st.deferred and self._representer_weights is None and return_var
        if not fuse:
            st.flush()
        rhs = self._cross(pts)
        pm = self._prior_mean_at(X if self.input_ndim else X[:, 0], X.shape[0])
        if fuse:
            self._ensure_residual()
            kxx = np.full(X.shape[0], self._prior_diag())
            out = rhs.potrf_predict(pm, kxx)          # (a failing call leaves the block deferred: nothing has been factored -- or the matrix is marked undefined)
            st.deferred, st.deferred_rows = False, 0
            return out
        if return_var and self._representer_weights is None:
            self._ensure_residual()
        else:
            self._ensure_weights()
        kxx = np.full(X.shape[0], self._prior_diag()) if return_var else None
        return rhs.predict(pm, kxx, want_mean=True, want_var=return_var)

    def var(self, x):
        return self.predict(x, return_var=True)[1]

    def log_marginal_likelihood(self) -> float:
        """log p(Y) = -1/2 r^T G^{-1} r - 1/2 log det G - n/2 log 2 pi of the observations this posterior was conditioned on,
        r = Y - L[m] - b.mean over all its blocks (the residual of the representer weights), G the Gram matrix with the
        noise.  Read off the resident factor (`lpgp_mat_evidence`): one forward solve and one reduction on the device, 16
        bytes back.  An earlier posterior of a chain answers for its own blocks (through its view).  Lazy mode: deferred
        factorisations are flushed and verified first, as `mean` does; a dropped block raises `LinAlgError`."""
        if not self._blocks:
            return 0.0
        _evidence_context("log_marginal_likelihood")
        self._check_current()
        r = self._residual()
        quad, logdet = self._state.mat.evidence(r)
        return float(-0.5 * quad - 0.5 * logdet - 0.5 * r.size * np.log(2.0 * np.pi))

    def leave_one_out(self) -> "LeaveOneOut":
        """Leave-one-out predictive distribution of every observation (`LeaveOneOut`): mean_i = y_i - w_i / d_i, var_i = 1 / d_i,
        log p_i = 1/2 log d_i - 1/2 w_i^2 / d_i - 1/2 log 2 pi with w = G^{-1} r and d = diag(G^{-1}), all formed on the device
        (`lpgp_mat_loo`; O(n) numbers cross the bus).  Shows which collocation or boundary points the model explains badly.
        Flushes, verifies and raises as `log_marginal_likelihood`."""
        if not self._blocks:
            return LeaveOneOut(np.zeros(0), np.zeros(0), np.zeros(0), 0.0)
        _evidence_context("leave_one_out")
        self._check_current()
        return LeaveOneOut(*self._state.mat.loo(self._residual(), np.concatenate([ob.Y for ob in self._blocks])))

    def cross_validate(self, folds, *, return_cov: bool = False) -> "FoldPredictions":
        """Leave-fold-out cross-validation (`FoldPredictions`): the predictive distribution of every fold B of observations given
        all the others, mean_B = y_B - S^{-1} w_B, Sigma_B = S^{-1}, log p(y_B | y_-B) = -1/2 w_B^T S^{-1} w_B + 1/2 log det S
        - |B|/2 log 2 pi with S = G^{-1}[B, B] and w = G^{-1} r (GPML section 5.4.2) -- "leave this boundary edge out", "leave every
        8th collocation point out together" without a conditioning per fold.  `folds`: "blocks" (one fold per observation block of
        the chain), an int k (row i of the Gram order goes to fold i % k) or a sequence of disjoint 1-D index arrays in Gram order
        that need not cover all rows (`_normalise_folds`).  G^{-1} is formed once on the device from the resident factor
        (`lpgp_mat_inverse`) and released at the end; the folds are reduced there (`lpgp_mat_cv`, csrc/evidence_cv.hip), O(n)
        numbers cross the bus, and the covariances with `return_cov`.  Singleton folds are `leave_one_out()`, one fold of all rows
        is `log_marginal_likelihood()`.  An earlier posterior of a chain answers for its own blocks; flushes, verifies and raises
        as `leave_one_out`."""
        if not self._blocks:
            raise ValueError("`cross_validate` needs observations: this process has been conditioned on none")
        fold_of, lists = _normalise_folds(folds, [ob.rows for ob in self._blocks])
        _evidence_context("cross_validate")
        self._check_current()
        mat = self._state.mat
        r, y = self._residual(), np.concatenate([ob.Y for ob in self._blocks])
        ginv = mat.inverse()
        try:
            mean, var, logp, total, cov = mat.cv(ginv, r, y, fold_of, len(lists), return_cov=bool(return_cov))
        finally:
            del ginv
        return FoldPredictions(lists, mean, var, logp, total, cov)

    def log_marginal_likelihood_gradient(self) -> "EvidenceGradient":
        """The log marginal likelihood and its gradient by the log hyperparameters of the prior covariance and of the noise
        (`EvidenceGradient`): 1/2 w^T dG w - 1/2 tr(G^{-1} dG) per parameter (GPML eq. 5.9), analytic -- differencing
        `log_marginal_likelihood()` over fresh conditionings loses most digits at the condition numbers of these Gram matrices.
        G^{-1} is formed once on the device from the resident factor (`lpgp_mat_inverse`) and released at the end; every dG is
        assembled into ONE scratch matrix by replaying the chain's block rows with a derived descriptor and no noise -- one summand
        alone (output scale), one summand with `dlog_lengthscale` set (lengthscale) -- and contracted in one streaming pass
        (`lpgp_mat_evidence_grad`); a diagonal noise needs no matrix (`lpgp_mat_evidence_grad_diag`).  Three n x n matrices are
        alive at most.  An earlier posterior of a chain answers for its own blocks; flushes, verifies and raises as
        `log_marginal_likelihood`.  An isotropic multivariate Matern prior raises `NotImplementedError` (no closed form of its
        lengthscale derivative here; use a `TensorProduct` prior), and so does a prior with a Wendland summand."""
        if _has_variable(self._blocks):
            raise NotImplementedError(f"`log_marginal_likelihood_gradient` is not available on a chain with {_VARIABLE} yet")
        if _has_mixed(self._blocks):
            raise NotImplementedError(f"`log_marginal_likelihood_gradient` is not available on a chain with {_MIXED} yet")
        base = self._prior.cov
        base_groups = covfuncs._base(base)._base_groups()
        G, d = len(base_groups), max(int(np.prod(self._prior.input_shape, dtype=int)), 1)
        if not self._blocks:
            return EvidenceGradient(0.0, np.zeros(G), np.zeros((G, d)), np.zeros(0))
        ctx = _evidence_context("log_marginal_likelihood_gradient")
        if any(f[0][0] == covfuncs.MATERN_ISO for _, f in base_groups):
            raise NotImplementedError("`log_marginal_likelihood_gradient` is not available for the isotropic multivariate Matérn kernel "
                                      "(its lengthscale derivative has no closed form here); use a `TensorProduct` prior")
        if any(f[0] in (covfuncs.WENDLAND, covfuncs.WENDLAND_ISO) for _, fs in base_groups for f in fs):
            raise NotImplementedError("`log_marginal_likelihood_gradient` is not available for a prior with a Wendland summand "
                                      "(the lengthscale derivative of the Wendland families is not built)")
        self._check_current()
        mat = self._state.mat
        r = self._residual()
        quad, logdet = mat.evidence(r)
        value = float(-0.5 * quad - 0.5 * logdet - 0.5 * r.size * np.log(2.0 * np.pi))
        blocks = self._blocks
        # descriptor groups of every block pair (i, j <= i), once: the derived descriptors pick from them
        pair = [[covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(base), *_combine(base, bi.coeffs, bj.coeffs)).lower()
                 for bj in blocks[:i + 1]] for i, bi in enumerate(blocks)]
        ginv = mat.inverse()
        scratch = _engine.GramMatrix(ctx, capacity_hint=mat.padded_n)

        def contract(derive, dense_block=None, dense=None) -> float:
            """1/2 w^T dG w - 1/2 tr(G^{-1} dG) for dG = the chain's block rows under `derive(groups)` (+ `dense` on one block)."""
            try:
                for i, bi in enumerate(blocks):
                    row = [(derive(pair[i][j]), bj.points) for j, bj in enumerate(blocks[:i])]
                    row.append((derive(pair[i][i]), None))
                    info = scratch.condition(bi.rows, bi.points, row, noise_dense=dense if i == dense_block else None, lazy=2)
                    assert info == 0
                q, t = mat.evidence_grad(ginv, scratch, r)
            finally:
                scratch.truncate(0)
            return 0.5 * q - 0.5 * t

        try:
            d_scale, d_ls, d_noise = np.zeros(G), np.zeros((G, d)), np.zeros(len(blocks))
            for g in range(G):
                d_scale[g] = contract(lambda groups, g=g: [groups[g]])
                for j in range(d):
                    d_ls[g, j] = contract(lambda groups, g=g, j=j: [dict(groups[g], dlog_lengthscale=j + 1)])
            for b, ob in enumerate(blocks):
                scalar, diag, dense = _block_noise(ob)
                if dense is not None:
                    d_noise[b] = contract(lambda groups: [dict(groups[0], scale=0.0)], b, dense)
                elif diag is not None or scalar != 0.0:
                    q, t = mat.evidence_grad_diag(ginv, b, r, v=diag, scalar=scalar)
                    d_noise[b] = 0.5 * q - 0.5 * t
        finally:
            del scratch, ginv
        return EvidenceGradient(value, d_scale, d_ls, d_noise)

    def sample(self, rng, x, size=(), *, damping=None):
        """Joint draws of the posterior (of the read-out `D(u)` if this object is one) at the points `x`.

        Shapes and the random stream as `GaussianProcess.sample`: `x` of shape batch + input_shape, result size + batch,
        exactly one call `z = rng.standard_normal(size + (M,))`, points flattened in C order, `draw[s] = mean(x) + C z[s]`
        with `C C^T = Sigma(x, x) + delta I`, `delta = damping *` (prior variance of the sampled field).  `Sigma(x, x) =
        k(x, x) - V^T V`, `V = L^{-1} K_Xx` (`_conditional.py:223-231`), is formed in a device matrix of its own
        (`lpgp_mat_sub_inner`) and factored there; the M x M covariance never visits the host, and the posterior's Gram
        matrix is neither extended nor copied: a posterior is a value, sampling changes nothing observable.  The factor of
        the last point set (points by value, damping, read-out) is kept: more draws at the same points cost one product.
        Lazy mode: a deferred factorisation is flushed and verified first, as `cov.matrix` does."""
        size = _sample_size(size)
        damping = _sample_damping(damping)
        X, batch = _sample_points(self, x)
        M = X.shape[0]
        z = np.asarray(rng.standard_normal(size + (M,)), dtype=np.double)
        if z.shape != size + (M,):
            raise ValueError(f"`rng.standard_normal` returned shape {z.shape}, expected {size + (M,)}")
        if M == 0:
            return np.empty(size + batch)
        _sample_context()
        self._check_current()
        ctx = self._state.ctx
        delta = damping * self._prior_diag()
        key = tuple(sorted(self._test_coeffs.items()))
        hit = _cached_factor(self, X, delta, key)
        if hit is None:
            mean = np.array(self.predict(x, return_var=False), dtype=np.double).reshape(-1)
            self._check_current()
            P = _engine.Points(ctx, X)
            S = _engine.GramMatrix(ctx, capacity_hint=M)
            S.add_block(M)
            S.assemble(_lowered(self._prior.cov, self._test_coeffs, self._test_coeffs), P, None, 0, 0)
            if self._blocks:
                V = self._cross(P)
                V.trsm_lower()
                S.sub_inner(0, V)
                del V
            _factor_damped(S, delta, damping)
            self._sample_cache = ((_engine.option_epoch(), delta, key), X.copy(), S, mean)
            hit = (S, mean)
        return _draws(hit[0], hit[1], z, size, batch)

    def __call__(self, x) -> randvars.Normal:
        X, batch = self._flat(x)
        if len(batch) != 1:
            raise ValueError("`__call__` needs inputs of shape (N,) + input_shape")
        return randvars.Normal(self.mean(x), self.cov.matrix(x))


_LOWERED: dict = {}      # (id(base), operator maps) -> (base, descriptor array); bounded, see _lowered


def _lowered(base, c0: dict, c1: dict):
    """C-ABI descriptor of the block  L0 (base) L1'^*, cached: composing the operator maps, lowering and filling the ctypes
    array cost ~25 us of Python per block -- a third of a whole step at N_tot ~ 1 000 -- and a chain of conditionings asks
    for the same few combinations every time.  Kernels are immutable; the entry keeps `base` alive so that its id cannot be
    reused while the entry exists."""
    key = (id(base), tuple(sorted(c0.items())), tuple(sorted(c1.items())))
    hit = _LOWERED.get(key)
    if hit is not None and hit[0] is base:
        return hit[1]
    k = covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(base), *_combine(base, c0, c1))
    arr = _engine.lowered_array(k.lower())
    if len(_LOWERED) >= 512:
        _LOWERED.clear()
    _LOWERED[key] = (base, arr)
    return arr


def _combine(base_cov, c0: dict, c1: dict):
    """Operator maps (arg 0, arg 1) of  L0 (base_cov) L1'^*  given the maps already on base_cov."""
    k0, k1 = base_cov._operator_coeffs()
    return covfuncs._compose(c0, k0), covfuncs._compose(c1, k1)


class _PosteriorMean(functions.Function):
    """`ConditionalGaussianProcess.Mean` (`_conditional.py:177-204`)."""

    def __init__(self, cgp: ConditionalGaussianProcess):
        super().__init__(input_shape=cgp._prior.input_shape, output_shape=())
        self._cgp = cgp

    def _evaluate(self, x):
        return self._cgp.predict(x, return_var=False)


class _PosteriorCovarianceFunction(covfuncs.CovarianceFunction):
    """`ConditionalGaussianProcess.CovarianceFunction` (`_conditional.py:206-251`)."""

    def __init__(self, cgp: ConditionalGaussianProcess):
        super().__init__(cgp._prior.input_shape)
        self._cgp = cgp

    def _base_groups(self):
        raise NotImplementedError("a posterior covariance function has no closed-form descriptor")

    def matrix(self, x0, x1=None) -> np.ndarray:
        cgp = self._cgp
        cgp._check_current()
        X0, b0 = cgp._flat(x0)
        if len(b0) != 1:
            raise ValueError("`matrix` needs inputs of shape (N,) + input_shape")
        ctx = cgp._state.ctx
        base = cgp._prior.cov
        kxx_f = covfuncs.DifferentiatedCovarianceFunction(
            covfuncs._base(base), *_combine(base, cgp._test_coeffs, cgp._test_coeffs))
        X1 = X0
        if x1 is not None:
            X1, b1 = cgp._flat(x1)
            if len(b1) != 1:
                raise ValueError("`matrix` needs inputs of shape (N,) + input_shape")
        if X0.shape[0] == 0 or X1.shape[0] == 0:
            return np.zeros((X0.shape[0], X1.shape[0]))
        P0 = _engine.Points(ctx, X0)
        P1 = P0 if x1 is None else _engine.Points(ctx, X1)
        k_xx = _engine.kernel_matrix(ctx, kxx_f.lower(), P0, P1)
        if not cgp._blocks:                       # nothing observed yet: the prior covariance
            return k_xx
        V0 = cgp._cross(P0)
        V0.trsm_lower()
        if x1 is None:
            V1 = V0
        else:
            V1 = cgp._cross(P1)
            V1.trsm_lower()
        return k_xx - V0.inner(V1)

    def linop(self, x0, x1=None) -> "PosteriorCovarianceOperator":
        """The posterior covariance between two point sets AS A LINEAR OPERATOR (`_conditional.py:245-251`:
        `k_xx - kLas_x0 @ gram.solve(kLas_x1.T)` built from probnum linear operators): products run on the device and the
        n0 x n1 matrix never exists; `.T` and `todense()` as the callers of a `LinearOperator` expect."""
        return PosteriorCovarianceOperator(self._cgp, x0, x1)

    def __call__(self, x0, x1=None):
        if x1 is None:
            return self._cgp.var(x0)
        X0, b0 = self._cgp._flat(x0)
        X1, b1 = self._cgp._flat(x1)
        out_shape = np.broadcast_shapes(b0, b1)
        K = self.matrix(X0 if self.input_ndim else X0[:, 0], X1 if self.input_ndim else X1[:, 0])
        i0 = np.broadcast_to(np.arange(X0.shape[0]).reshape(b0), out_shape)
        i1 = np.broadcast_to(np.arange(X1.shape[0]).reshape(b1), out_shape)
        return K[i0, i1]


class PosteriorCovarianceOperator:
    """`Sigma(x0, x1) = k(x0, x1) - K_x0X G^{-1} K_Xx1` as a matrix-free operator (`_conditional.py:245-251`).

    Resident on the device: V0 = L^{-1} K_Xx0 and V1 = L^{-1} K_Xx1 (one forward substitution each, at construction; the same
    block when x1 is x0).  A product is  k(x0, x1) @ V  -- every kernel entry evaluated on the fly, `lpgp_kernel_matvec` --
    minus  V0^T (V1 V)  -- two MFMA products, `lpgp_rhs_matmul` and `lpgp_rhs_inner`: O((n0 + n1) N m) work and no n0 x n1
    array anywhere.  The operator is a value like the posterior it belongs to: later conditionings of that posterior do not
    change it."""

    def __init__(self, cgp: "ConditionalGaussianProcess", x0, x1=None, _parts=None):
        self.dtype = np.dtype(np.double)
        if _parts is not None:
            self._kop, self._V0, self._V1, self.shape = _parts
            return
        cgp._check_current()
        X0, b0 = cgp._flat(x0)
        X1, b1 = (X0, b0) if x1 is None else cgp._flat(x1)
        if len(b0) != 1 or len(b1) != 1:
            raise ValueError("`linop` needs inputs of shape (N,) + input_shape")
        base = cgp._prior.cov
        kxx_f = covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(base), *_combine(base, cgp._test_coeffs, cgp._test_coeffs))
        a0 = X0 if cgp.input_ndim else X0[:, 0]
        a1 = a0 if x1 is None else (X1 if cgp.input_ndim else X1[:, 0])
        self._kop = covfuncs.KernelLinearOperator(kxx_f, a0, a1)
        self.shape = (X0.shape[0], X1.shape[0])
        self._V0 = self._V1 = None
        if cgp._blocks and X0.shape[0] and X1.shape[0]:
            self._V0 = cgp._cross(self._kop._P0)
            self._V0.trsm_lower()
            if x1 is None:
                self._V1 = self._V0
            else:
                self._V1 = cgp._cross(self._kop._P1)
                self._V1.trsm_lower()

    def __matmul__(self, V):
        V = np.asarray(V, dtype=np.double)
        if V.ndim not in (1, 2) or V.shape[0] != self.shape[1]:
            raise ValueError(f"shape mismatch: {self.shape} @ {V.shape}")
        V2 = V[:, None] if V.ndim == 1 else V
        if self.shape[0] == 0 or self.shape[1] == 0 or V2.shape[1] == 0:
            return np.zeros((self.shape[0],) + V.shape[1:])
        out = self._kop @ V2
        if self._V0 is not None:
            out = out - self._V0.inner(self._V1.matmul(V2))
        return out[:, 0] if V.ndim == 1 else out

    matmul = __matmul__

    @property
    def T(self) -> "PosteriorCovarianceOperator":
        return PosteriorCovarianceOperator(None, None, _parts=(self._kop.T, self._V1, self._V0, self.shape[::-1]))

    def todense(self) -> np.ndarray:
        K = self._kop.todense()
        return K if self._V0 is None else K - self._V0.inner(self._V1)


# ---- L(posterior) read-outs (`_conditional.py:432-467`) -------------------------------------
def apply_linfuncop_to_conditional_gp(L, cgp: ConditionalGaussianProcess) -> ConditionalGaussianProcess:
    cgp._check_current()
    coeffs = covfuncs._compose(L.coefficients_dict(), cgp._test_coeffs)
    cgp._ensure_weights()
    return ConditionalGaussianProcess(
        prior=cgp._prior, blocks=cgp._blocks, state=cgp._state,
        representer_weights=cgp._representer_weights, test_coeffs=coeffs)


def apply_linfunctl_to_conditional_gp(L, cgp: ConditionalGaussianProcess) -> randvars.Normal:
    cgp._ensure_weights()
    view = ConditionalGaussianProcess(
        prior=cgp._prior, blocks=cgp._blocks, state=cgp._state,
        representer_weights=cgp._representer_weights,
        test_coeffs=covfuncs._compose(L.coefficients_dict(), cgp._test_coeffs))
    X = L.points()
    x = X if cgp.input_ndim else X[:, 0]
    return randvars.Normal(view.mean(x), view.cov.matrix(x))


def apply_linfunctl_to_gp(L, gp: GaussianProcess) -> randvars.Normal:
    """`L(prior)`: joint law of L[f]  (`_lintransforms.py:9-22`)."""
    c = L.coefficients_dict()
    k = covfuncs.DifferentiatedCovarianceFunction(covfuncs._base(gp.cov), *_combine(gp.cov, c, c))
    X = L.points()
    x = X if gp.input_ndim else X[:, 0]
    mean = np.asarray(L(gp.mean), dtype=np.double).reshape(-1)
    return randvars.Normal(mean, k.matrix(x))
