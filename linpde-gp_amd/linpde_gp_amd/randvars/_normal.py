"""Minimal `Normal` / `Constant` random variables (probnum `randvars` protocol: `.mean`,
`.cov`, `.var`, `.std`, `.shape`), used for observation noise `b` and as the result type
of `GaussianProcess.__call__`."""

from __future__ import annotations

import numpy as np


class Normal:
    """Multivariate normal.  `cov` may be dense (n x n), a scalar (sigma^2 I) or a vector of
    variances (diagonal covariance, kept as a vector: a noisy block of 10^4+ observations
    must not materialise n^2 zeros)."""

    def __init__(self, mean, cov):
        self._mean = np.asarray(mean, dtype=np.double)
        cov = np.asarray(cov, dtype=np.double)
        n = self._mean.size
        self._cov_diag = None
        self._cov = None
        if self._mean.ndim == 0:
            self._cov = cov.reshape(())
        elif cov.ndim == 0:
            self._cov_diag = np.full(n, float(cov))
        elif cov.ndim == 1:
            if cov.shape != (n,):
                raise ValueError(f"variance vector has shape {cov.shape}, expected {(n,)}")
            self._cov_diag = cov.copy()
        elif cov.shape == (n, n):
            self._cov = cov
        else:
            raise ValueError(f"covariance has shape {cov.shape}, expected {(n, n)}")

    @property
    def mean(self):
        return self._mean

    @property
    def cov(self):
        if self._cov is None:
            self._cov = np.diag(self._cov_diag)
        return self._cov

    @property
    def cov_diag(self):
        """Variances if the covariance is (known to be) diagonal, else None."""
        return self._cov_diag

    @property
    def var(self):
        if self._cov_diag is not None:
            return self._cov_diag.reshape(self._mean.shape)
        if self._cov.ndim == 0:
            return self._cov
        return np.diag(self._cov).reshape(self._mean.shape)

    @property
    def std(self):
        return np.sqrt(np.maximum(self.var, 0.0))

    @property
    def shape(self):
        return self._mean.shape

    @property
    def size(self):
        return self._mean.size

    def _device_factor(self):
        """The dense covariance as a factored device matrix (`lpgp_mat_add_dense`, `lpgp_potrf`), built once."""
        S = getattr(self, "_cov_factor", None)
        if S is None:
            from .. import _engine, _spawn
            from ..randprocs import covfuncs
            if _spawn.active() is not None:
                raise NotImplementedError("`cov_cholesky` / `sample` are not available through the `lp.spawn` multi-GPU front")
            ctx = _engine.default_context()
            if ctx.distributed:
                raise NotImplementedError("`cov_cholesky` / `sample` are not available in a multi-GPU job")
            n = self._mean.size
            S = _engine.GramMatrix(ctx, n)
            bi = S.add_block(n)
            S.assemble(covfuncs.Zero(()).lower(), _engine.Points(ctx, np.zeros((n, 1))), None, bi, bi)   # clear the block, then add the covariance
            S.add_dense(bi, np.ascontiguousarray(self._cov.reshape(n, n)))
            info = S.potrf()
            if info != 0:
                raise np.linalg.LinAlgError(f"{info}-th leading minor of the covariance is not positive definite")
            self._cov_factor = S
        return S

    @property
    def cov_cholesky(self) -> np.ndarray:
        """Dense lower Cholesky factor of the covariance (probnum `Normal.cov_cholesky`), cached.  A dense covariance is
        factored on the device; scalar and diagonal covariances are square roots on the host."""
        C = getattr(self, "_cov_cholesky", None)
        if C is None:
            if self._mean.ndim == 0:
                C = np.sqrt(self._cov)
            elif self._cov_diag is not None:
                C = np.diag(np.sqrt(self._cov_diag))
            else:
                C = self._device_factor().todense("factor")
            if np.any(np.isnan(C)):
                raise np.linalg.LinAlgError("the covariance has a negative variance")
            self._cov_cholesky = C
        return C

    def logpdf(self, x):
        """Log density at `x` (probnum `Normal.logpdf`): `x` of shape batch + self.shape, result of shape batch.
        -1/2 (x - mean)^T cov^{-1} (x - mean) - 1/2 log det cov - n/2 log 2 pi.  Scalar and diagonal covariances in closed form
        on the host (O(n), no device call); a dense covariance through its factored device matrix (`lpgp_mat_evidence`: one
        forward solve and one reduction per point of the batch)."""
        x = np.asarray(x, dtype=np.double)
        shape = tuple(self._mean.shape)
        nd = len(shape)
        if x.shape[x.ndim - nd:] != shape:
            raise ValueError(f"`x` has shape {x.shape}, expected batch + {shape}")
        batch = x.shape[:x.ndim - nd]
        n = self._mean.size
        r = (x - self._mean).reshape(batch + (n,))
        if nd == 0 or self._cov_diag is not None:
            var = np.reshape(self._cov, (1,)) if nd == 0 else self._cov_diag
            if np.any(var <= 0.0):
                raise np.linalg.LinAlgError("the covariance is not positive definite")
            return -0.5 * np.sum(r * r / var, axis=-1) - 0.5 * np.sum(np.log(var)) - 0.5 * n * np.log(2.0 * np.pi)
        if n == 0:
            return np.zeros(batch)
        S = self._device_factor()
        out = np.empty(batch)
        for idx in np.ndindex(*batch):
            quad, logdet = S.evidence(np.ascontiguousarray(r[idx]))
            out[idx] = -0.5 * quad - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
        return out[()]

    @property
    def entropy(self) -> float:
        """Differential entropy n/2 (1 + log 2 pi) + 1/2 log det cov (probnum `Normal.entropy`); the determinant of a dense
        covariance from the diagonal of its device factor (`lpgp_mat_evidence`)."""
        n = self._mean.size
        if self._mean.ndim == 0 or self._cov_diag is not None:
            var = np.reshape(self._cov, (1,)) if self._mean.ndim == 0 else self._cov_diag
            if np.any(var <= 0.0):
                raise np.linalg.LinAlgError("the covariance is not positive definite")
            logdet = float(np.sum(np.log(var)))
        else:
            logdet = self._device_factor().evidence(np.zeros(n))[1] if n else 0.0
        return float(0.5 * n * (1.0 + np.log(2.0 * np.pi)) + 0.5 * logdet)

    def sample(self, rng, size=()):
        """Draws of shape size + self.shape (probnum `Normal.sample(rng, size)`).  THE RANDOM STREAM IS PART OF THE CONTRACT:
        exactly one call `z = rng.standard_normal(size + self.shape)` and `draw[s] = mean + C z[s]` with the lower Cholesky
        factor `C` of the covariance (the mean flattened in C order).  A dense covariance is factored and multiplied on the
        device (`lpgp_potrf`, `lpgp_mat_factor_matmul`); scalar and diagonal ones are scaled on the host, no device call."""
        if isinstance(size, (int, np.integer)):
            size = (int(size),)
        size = tuple(int(k) for k in size)
        if any(k < 0 for k in size):
            raise ValueError(f"`size` must not be negative, got {size}")
        shape = tuple(self._mean.shape)
        z = np.asarray(rng.standard_normal(size + shape), dtype=np.double)
        if z.shape != size + shape:
            raise ValueError(f"`rng.standard_normal` returned shape {z.shape}, expected {size + shape}")
        if self._mean.ndim == 0 or self._cov_diag is not None:
            var = self._cov if self._mean.ndim == 0 else self._cov_diag.reshape(shape)
            if np.any(var < 0.0):
                raise ValueError("the covariance has a negative variance")
            return self._mean + np.sqrt(var) * z
        n = self._mean.size
        if n == 0 or z.size == 0:
            return np.empty(size + shape)
        out = self._device_factor().factor_matmul(np.ascontiguousarray(z.reshape(-1, n).T), self._mean.reshape(-1))
        return np.ascontiguousarray(out.T).reshape(size + shape)


class Constant:
    def __init__(self, support):
        self._support = np.asarray(support, dtype=np.double)

    @property
    def mean(self):
        return self._support

    @property
    def support(self):
        return self._support

    @property
    def cov(self):
        n = self._support.size
        return np.zeros((n, n))

    @property
    def shape(self):
        return self._support.shape


def asrandvar(b):
    if isinstance(b, (Normal, Constant)):
        return b
    if np.ndim(b) >= 0 and not hasattr(b, "mean"):
        return Constant(b)
    raise TypeError(f"`b` must be a `Normal` or a `Constant` `RandomVariable` ({type(b)=})")


def condition_normal_on_observations(prior: Normal, observations, noise: Normal | None = None, transform=None) -> Normal:
    r"""Finite-dimensional Gaussian conditioning (`randvars/_normal.py:8-71` of the reference):
    observe `y = A x + eps`, `x ~ N(mu0, Sigma0)`, `eps ~ N(b, Lambda)`.

    The Gram matrix `A Sigma0 A^T + Lambda` is factored on the device (`lpgp_potrf`) and the
    gain `Gram^{-1} (A Sigma0)` comes from ONE multi-right-hand-side solve (`lpgp_potrs`) -- the
    reference calls LAPACK `cho_solve` on the host.  Also bound as
    `Normal.condition_on_observations`."""
    from .. import _engine
    from ..randprocs import covfuncs

    observations = np.asarray(observations, dtype=np.double)
    A = None if transform is None else np.asarray(transform, dtype=np.double)
    if A is not None and A.ndim == 1:
        A = A[None, :]
        observations = observations.reshape(1)
        if noise is not None:
            noise = Normal(np.asarray(noise.mean).reshape(1), np.asarray(noise.cov).reshape(1, 1))
    mu0 = np.asarray(prior.mean, dtype=np.double).reshape(-1)
    S0 = np.asarray(prior.cov, dtype=np.double).reshape(mu0.size, mu0.size)
    ctx = _engine.default_context()
    # (the three dense products of the update run on the device's MFMA kernel since round 6 -- `lpgp_gemm_host`; NumPy until then)
    crosscov = S0 if A is None else _engine.gemm(ctx, A, S0)     # Cov(y, x), (n_obs, n)
    pred_mean = mu0 if A is None else A @ mu0
    pred_cov = S0 if A is None else _engine.gemm(ctx, crosscov, A, transb=True)
    if noise is not None:
        pred_mean = pred_mean + np.asarray(noise.mean, dtype=np.double).reshape(-1)
        pred_cov = pred_cov + np.asarray(noise.cov, dtype=np.double).reshape(pred_cov.shape)
    n_obs = pred_mean.size
    if observations.reshape(-1).size != n_obs:
        raise ValueError(f"expected {n_obs} observations, got shape {observations.shape}")
    mat = _engine.GramMatrix(ctx, n_obs)
    bi = mat.add_block(n_obs)
    pts = _engine.Points(ctx, np.zeros((n_obs, 1)))
    mat.assemble(covfuncs.Zero(()).lower(), pts, None, bi, bi)   # clear the block, then add the dense Gram
    mat.add_dense(bi, np.ascontiguousarray(pred_cov))
    info = mat.potrf()
    if info != 0:
        raise np.linalg.LinAlgError(f"{info}-th leading minor of the predictive covariance is not positive definite")
    # [gain^T | weights] = Gram^{-1} [crosscov | y - pred_mean] in one solve
    rhs = np.concatenate([crosscov, (observations.reshape(-1) - pred_mean)[:, None]], axis=1)
    sol = mat.potrs(rhs)
    gain_t, w = sol[:, :-1], sol[:, -1]
    return Normal(mean=(mu0 + crosscov.T @ w).reshape(np.shape(prior.mean)),
                  cov=_engine.gemm(ctx, crosscov, gain_t, transa=True, alpha=-1.0, beta=1.0, C=S0))


Normal.condition_on_observations = condition_normal_on_observations


