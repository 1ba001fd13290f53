"""The NumPy reference of the evidence / leave-one-out tests (tests/_evidence_reference.py) against brute force and against a
50-digit solve, and `Normal.logpdf` / `Normal.entropy` with scalar and diagonal covariances (closed forms on the host)
against SciPy.  No device."""
import mpmath
import numpy as np
import pytest
import scipy.stats

import _evidence_reference as ref


@pytest.fixture(scope="module")
def problem():
    return ref.Problem40()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_problem_is_well_conditioned(problem):
    assert np.linalg.cond(problem.G) < 1e4


def test_closed_form_loo_equals_brute_force(problem):
    """The criterion the GPU tolerances rest on: closed forms within 1e-10 (relative to max |ref|) of delete-refactor-predict."""
    mean, var, logp = ref.loo(problem.G, problem.r, problem.Y)
    bmean, bvar, blogp = ref.loo_brute_force(problem.G, problem.r, problem.Y)
    errs = _rel(mean, bmean), _rel(var, bvar), _rel(logp, blogp)
    print("closed form vs brute force (mean, var, logp):", errs)
    assert max(errs) < 1e-10, errs


def test_reference_equals_a_50_digit_solve(problem):
    n = problem.r.size
    with mpmath.workdps(50):
        G = mpmath.matrix(problem.G.tolist())
        r = mpmath.matrix(problem.r.tolist())
        Ginv = mpmath.inverse(G)
        w = Ginv * r
        quad = (r.T * w)[0]
        logdet = mpmath.log(mpmath.det(G))
        d = [Ginv[i, i] for i in range(n)]
        mean = np.array([float(mpmath.mpf(float(problem.Y[i])) - w[i] / d[i]) for i in range(n)])
        var = np.array([float(1 / d[i]) for i in range(n)])
        logp = np.array([float(mpmath.log(d[i]) / 2 - w[i] ** 2 / d[i] / 2 - mpmath.log(2 * mpmath.pi) / 2) for i in range(n)])
        lml = float(-quad / 2 - logdet / 2 - n * mpmath.log(2 * mpmath.pi) / 2)
        quad, logdet, diag = float(quad), float(logdet), np.array([float(v) for v in d])
    q, ld, l = ref.evidence(problem.G, problem.r)
    assert abs(q - quad) < 1e-10 * abs(quad) and abs(ld - logdet) < 1e-10 * abs(logdet) and abs(l - lml) < 1e-10 * abs(lml)
    assert _rel(ref.inverse_diag(problem.G), diag) < 1e-10
    m, v, lp_ = ref.loo(problem.G, problem.r, problem.Y)
    assert max(_rel(m, mean), _rel(v, var), _rel(lp_, logp)) < 1e-10


@pytest.mark.parametrize("shape", [(), (7,), (3, 4)])
def test_normal_logpdf_and_entropy_diagonal(shape):
    from linpde_gp_amd import randvars
    rng = np.random.default_rng(len(shape))
    mean = rng.standard_normal(shape)
    var = rng.uniform(0.1, 2.0, shape)
    n = mean.size
    N = randvars.Normal(mean, var if shape == () else var.reshape(-1))
    sp = scipy.stats.multivariate_normal(mean.reshape(-1), np.diag(var.reshape(-1)))
    x = rng.standard_normal((5,) + shape)
    got = N.logpdf(x)
    assert got.shape == (5,)
    np.testing.assert_allclose(got, sp.logpdf(x.reshape(5, n)), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(N.logpdf(x[0]), sp.logpdf(x[0].reshape(n)), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(N.entropy, sp.entropy(), rtol=1e-13)
    if shape:                                                 # (every array is a batch of scalars)
        with pytest.raises(ValueError):
            N.logpdf(np.zeros(shape + (2,)))


def test_normal_scalar_covariance_and_refusals():
    from linpde_gp_amd import randvars
    N = randvars.Normal(np.arange(4.0), 0.3)                  # sigma^2 I
    sp = scipy.stats.multivariate_normal(np.arange(4.0), 0.3 * np.eye(4))
    np.testing.assert_allclose(N.logpdf(np.ones(4)), sp.logpdf(np.ones(4)), rtol=1e-13)
    np.testing.assert_allclose(N.entropy, sp.entropy(), rtol=1e-13)
    with pytest.raises(np.linalg.LinAlgError):
        randvars.Normal(np.zeros(3), np.array([1.0, 0.0, 1.0])).logpdf(np.zeros(3))
    with pytest.raises(np.linalg.LinAlgError):
        randvars.Normal(np.zeros(3), np.array([1.0, -1.0, 1.0])).entropy
