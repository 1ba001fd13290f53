"""The dense reference of tests/test_gpu_mixed.py checks itself (no device): the matrix form of a block equals the literal double
loop over the stencils, the Gauss weights do what the problems need of them, and the two problems are well enough conditioned
that LAPACK's posterior on the reference Gram matrix stays within a quarter of the GPU test's tolerances from the posterior
refined in long double -- otherwise a parity failure there would say nothing about the device.

Measured: worst ratio to `posterior_tolerances` 0.03 (1-D, variance) and 0.006 (2-D, weights); condition numbers 4e5 and 5e8."""
import numpy as np
import pytest

import _mixed_reference as mr
from conftest import POSTERIOR_RTOL, posterior_tolerances


def test_reference_block_equals_the_literal_double_loop_over_the_stencils():
    rng = np.random.default_rng(7)
    kernel = [(1.3, [("matern", 2.5, 0.7), ("matern", 3.5, 0.9)])]
    X0, X1 = rng.uniform(-1, 1, (23, 2)), rng.uniform(-1, 1, (17, 2))
    idx0, w0 = rng.integers(0, 23, (9, 4)).astype(np.int32), rng.normal(size=(9, 4))
    idx1, w1 = rng.integers(0, 17, (6, 3)).astype(np.int32), rng.normal(size=(6, 3))
    w0[2, 1:] = 0.0
    idx0[2, 1:] = idx0[2, 0]                     # a padded row
    D0, D1 = {(2, 0): -1.0, (0, 2): -1.0}, {(0, 0): 1.0}
    ref, env, absw = mr.block(kernel, D0, D1, X0, X1, mr.dense_of(idx0, w0, 23), mr.dense_of(idx1, w1, 17))
    loop = mr.stencil_block(kernel, D0, D1, X0, X1, idx0, w0, idx1, w1)
    assert np.all(np.abs(ref - loop) <= 12 * 4 * np.finfo(float).eps * env + 1e-300)
    assert np.all(env <= absw * (1 + 1e-12)) and np.all(np.abs(ref) <= env * (1 + 1e-12))


def test_gauss_weights_integrate_a_cubic_exactly():
    edges = np.array([-1.0, -0.3, 0.1, 1.0])
    for npts in (2, 3):
        x, A = mr.gauss_cells_1d(edges, npts)
        p = lambda t: 2 * t ** 3 - t ** 2 + 0.5 * t - 3
        P = lambda t: 0.5 * t ** 4 - t ** 3 / 3 + 0.25 * t ** 2 - 3 * t
        exact = (P(edges[1:]) - P(edges[:-1])) / np.diff(edges)
        np.testing.assert_allclose(A @ p(x), exact, rtol=0, atol=8 * np.finfo(float).eps * 4)
        np.testing.assert_allclose(A.sum(axis=1), 1.0, rtol=0, atol=4 * np.finfo(float).eps)


def _problems():
    k1, o1, x1 = mr.problem_1d("boundary first")
    k2, o2, x2 = mr.problem_2d()
    return [("1d", k1, o1, x1), ("2d", k2, o2, x2)]


@pytest.mark.parametrize("which", [0, 1], ids=["1d", "2d"])
def test_lapack_posterior_is_well_within_the_parity_tolerances(which):
    name, kernel, obs, Xt = _problems()[which]
    ref = mr.Reference(kernel, obs)
    assert ref.G.shape[0] == sum(o.rows for o in obs) == (142 if which == 0 else 204)
    mean, var = ref.predict(Xt)
    rmean, rvar, rw = ref.refined(Xt)
    mean_atol, var_atol = posterior_tolerances(rmean, rvar)
    ratios = (np.max(np.abs(mean - rmean)) / mean_atol, np.max(np.abs(var - rvar)) / var_atol,
              np.max(np.abs(ref.w - rw)) / (POSTERIOR_RTOL * np.max(np.abs(rw))))
    print(name, "cond", np.linalg.cond(ref.G), "ratios (mean, var, weights)", ratios)
    assert max(ratios) <= 0.25
