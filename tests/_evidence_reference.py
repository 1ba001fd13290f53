"""NumPy reference for the model evidence and the leave-one-out (LOO) predictive distributions of a GP, by the closed forms
the library implements (Rasmussen & Williams, GPML eq. 2.30 and eqs. 5.10 - 5.12), the brute-force LOO they are checked
against (tests/test_evidence_host.py), and the one small noisy problem both test files share.  Host only."""
import numpy as np
import scipy.linalg

from oracle import covfuncs as ocf

LOG_2PI = float(np.log(2.0 * np.pi))


def evidence(G, r):
    """(r^T G^-1 r, log det G, log marginal likelihood) through the Cholesky factor of G."""
    chol = scipy.linalg.cholesky(G, lower=True)
    z = scipy.linalg.solve_triangular(chol, r, lower=True)
    quad = float(z @ z)
    logdet = float(2.0 * np.sum(np.log(np.diag(chol))))
    return quad, logdet, -0.5 * quad - 0.5 * logdet - 0.5 * r.size * LOG_2PI


def inverse_diag(G):
    chol = scipy.linalg.cholesky(G, lower=True)
    Linv = scipy.linalg.solve_triangular(chol, np.eye(G.shape[0]), lower=True)
    return np.sum(Linv * Linv, axis=0)


def loo(G, r, y):
    """LOO (mean, var, logp) of every noisy observation: r = y - (prior predictive mean), G = Gram + noise."""
    d = inverse_diag(G)
    w = scipy.linalg.cho_solve(scipy.linalg.cho_factor(G, lower=True), r)
    return y - w / d, 1.0 / d, 0.5 * np.log(d) - 0.5 * w * w / d - 0.5 * LOG_2PI


def loo_brute_force(G, r, y):
    """The same numbers the long way: delete row and column i, refactor, predict observation i from the others."""
    n = r.size
    mean, var = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        cf = scipy.linalg.cho_factor(G[np.ix_(keep, keep)], lower=True)
        g = G[keep, i]
        mean[i] = (y[i] - r[i]) + g @ scipy.linalg.cho_solve(cf, r[keep])
        var[i] = G[i, i] - g @ scipy.linalg.cho_solve(cf, g)
    return mean, var, -0.5 * (y - mean) ** 2 / var - 0.5 * np.log(var) - 0.5 * LOG_2PI


class Problem40:
    """40 scattered 1-D points, prior 0.5 + GP(1.3 Matern-5/2, l = 0.5), heteroscedastic noise of 1e-2 .. 3e-2 with a
    non-zero mean: cond_2(G) ~ 1e3, so the closed forms and the brute force agree far below the 1e-10 the tests ask."""
    kernel = [(1.3, [("matern", 2.5, 0.5)])]
    mean_const = 0.5

    def __init__(self):
        rng = np.random.default_rng(40)
        self.X = np.sort(rng.uniform(-1.0, 1.0, 40))[:, None]
        self.noise_var = rng.uniform(1e-2, 3e-2, 40)
        self.noise_mean = 0.05 * rng.standard_normal(40)
        self.Y = 0.5 + np.sin(3.0 * self.X[:, 0]) + self.noise_mean + np.sqrt(self.noise_var) * rng.standard_normal(40)
        ident = ocf.identity(1)
        self.G = ocf.LkL(self.kernel, ident, ident, self.X, self.X) + np.diag(self.noise_var)
        self.r = self.Y - self.mean_const - self.noise_mean
