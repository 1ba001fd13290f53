"""Observations through a matrix, `A @ L`, without a device: the Python surface (`linfunctls.LinearFunctional.__rmatmul__`,
`CompositeLinearFunctional(linop=...)`, `mixing()`), the refusals that need no GPU by their messages, and the stencil-table header
`csrc/mix_table.h` under AddressSanitizer + UBSan through the stand-alone program `csrc/hosttest/mix_check.cpp` (nothing is
loaded into Python)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse

import linpde_gp_amd as lp
from linpde_gp_amd import linfunctls
from linpde_gp_amd.linfuncops import diffops

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "linpde-gp_amd", "csrc")


def _ev(n=7, d=2, seed=0):
    X = np.random.default_rng(seed).uniform(-1, 1, (n, d))
    return linfunctls._EvaluationFunctional((d,), (), X), X


def _same(L1, L2, ulps=0):
    """The same functional: points, coefficient map, stencils; `ulps`: slack of the weights where the two sides multiply the
    matrices in different orders of summation (a sparse against a dense product)."""
    i1, w1 = L1.mixing()
    i2, w2 = L2.mixing()
    return (np.array_equal(L1.points(), L2.points()) and L1.coefficients_dict() == L2.coefficients_dict() and np.array_equal(i1, i2)
            and bool(np.all(np.abs(w1 - w2) <= ulps * np.finfo(float).eps * np.abs(w2).max())) and L1.output_shape == L2.output_shape)


def test_rmatmul_builds_a_composite_with_the_matrix_rows_as_output():
    ev, X = _ev()
    A = np.zeros((3, 7))
    A[0, [1, 4]] = [0.5, 0.5]
    A[1, 2] = -2.0
    A[2, [0, 3, 6]] = [1.0, -2.0, 1.0]
    L = A @ ev
    assert isinstance(L, linfunctls.CompositeLinearFunctional) and L.linop is not None
    assert L.output_shape == (3,) and L.output_size == 3 and L.input_shapes == ev.input_shapes
    assert np.array_equal(L.points(), X) and L.coefficients_dict() == {(0, 0): 1.0}
    assert ev.mixing() is None and (2.0 * ev).mixing() is None and (ev @ diffops.Laplacian((2,))).mixing() is None
    with pytest.raises(ValueError, match="does not match"):
        np.zeros((3, 6)) @ ev
    with pytest.raises(TypeError):
        np.zeros(7) @ ev                          # a vector is no mixing matrix


def test_mixing_packs_ragged_rows_in_column_order_with_the_padding_rule():
    ev, _ = _ev()
    A = np.zeros((4, 7))
    A[0, [4, 1]] = [0.25, 0.75]
    A[1, 2] = -2.0
    A[3, [6, 0, 3]] = [1.0, 3.0, -2.0]           # row 2 stays empty
    idx, w = (A @ ev).mixing()
    assert idx.dtype == np.int32 and w.dtype == np.double and idx.shape == w.shape == (4, 3)
    assert np.array_equal(idx, [[1, 4, 1], [2, 2, 2], [0, 0, 0], [0, 3, 6]])
    assert np.array_equal(w, [[0.75, 0.25, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [3.0, -2.0, 1.0]])
    # a scipy.sparse input gives the same table, stored zeros and unsorted indices included
    S = scipy.sparse.csr_matrix((np.array([0.25, 0.75, 0.0, -2.0, 1.0, 3.0, -2.0]), np.array([4, 1, 5, 2, 6, 0, 3]), np.array([0, 3, 4, 4, 7])), shape=(4, 7))
    Ls = S @ ev
    assert Ls.output_shape == (4,)
    idx_s, w_s = Ls.mixing()
    assert np.array_equal(idx_s, idx) and np.array_equal(w_s, w)
    assert np.array_equal((scipy.sparse.coo_matrix(A) @ ev).mixing()[1], w)


def test_composition_laws_and_scaling():
    ev, _ = _ev()
    rng = np.random.default_rng(1)
    A1 = np.where(rng.uniform(size=(5, 7)) < 0.4, rng.normal(size=(5, 7)), 0.0)
    A2 = np.where(rng.uniform(size=(3, 5)) < 0.6, rng.normal(size=(3, 5)), 0.0)
    D = diffops.Laplacian((2,))
    # A2 @ (A1 @ L) == (A2 A1) @ L
    assert _same(A2 @ (A1 @ ev), (A2 @ A1) @ ev)
    assert _same(scipy.sparse.csr_matrix(A2) @ (A1 @ (ev @ D)), (A2 @ A1) @ (ev @ D), ulps=8)
    # (A @ ev) @ D == A @ (ev @ D)
    assert _same((A1 @ ev) @ D, A1 @ (ev @ D))
    assert ((A1 @ ev) @ D).coefficients_dict() == (ev @ D).coefficients_dict()
    # a scalar scales the weights, not the coefficient map
    L = -2.5 * (A1 @ (ev @ D))
    assert _same(L, (-2.5 * A1) @ (ev @ D))
    assert _same(-(A1 @ ev), (-A1) @ ev)
    # a matrix in front of a scaled functional: the scalar stays in the coefficient map
    L = A1 @ (3.0 * ev)
    assert L.coefficients_dict() == {(0, 0): 3.0} and np.array_equal(L.mixing()[1], (A1 @ ev).mixing()[1])


def test_application_to_a_function_is_the_matrix_times_the_flattened_values():
    ev, X = _ev()
    A = np.random.default_rng(2).normal(size=(3, 7)) * (np.arange(21).reshape(3, 7) % 3 == 0)
    f = lp.functions.LambdaFunction(lambda x: np.sin(x[..., 0]) * x[..., 1], (2,))
    vals = np.sin(X[:, 0]) * X[:, 1]
    np.testing.assert_allclose((A @ ev)(f), A @ vals, rtol=0, atol=1e-15)
    np.testing.assert_allclose((scipy.sparse.csr_matrix(A) @ ev)(f), A @ vals, rtol=0, atol=1e-15)
    # over a batch of points of shape (2, 3): the matrix acts on the C-order flattening
    Xb = np.random.default_rng(3).uniform(-1, 1, (2, 3, 2))
    evb = linfunctls._EvaluationFunctional((2,), (), Xb)
    B = np.arange(12.0).reshape(2, 6)
    np.testing.assert_allclose((B @ evb)(f), B @ (np.sin(Xb[..., 0]) * Xb[..., 1]).reshape(-1), rtol=0, atol=1e-14)
    zero = lp.functions.Zero((2,))
    assert np.array_equal(np.asarray((A @ ev)(zero), dtype=float).reshape(-1), np.zeros(3))


def test_refusals_name_the_feature_or_the_limit(monkeypatch):
    from linpde_gp_amd import _spawn, config
    ev, X = _ev(40)
    A = np.zeros((2, 40))
    A[0, :33] = 1.0
    A[1, 3] = 1.0
    with pytest.raises(NotImplementedError, match="33 non-zeros, more than LPGP_MAXS = 32"):
        (A @ ev).mixing()
    A[0, 32] = 0.0
    assert (A @ ev).mixing()[0].shape == (2, 32)            # exactly the cap passes
    V = diffops.VariableCoefficientOperator((2,), [(lp.functions.LambdaFunction(lambda x: 1 + x[..., 0] ** 2, (2,)), diffops.Laplacian((2,)))])
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator.*under a leading matrix factor"):
        (A @ V.to_linfunctl(X)).variable_terms()
    with pytest.raises(NotImplementedError, match="sum of functionals with a leading matrix factor"):
        ((A @ ev) + (A @ ev)).mixing()
    prior = lp.GaussianProcess(lp.functions.Zero((2,)), lp.randprocs.covfuncs.TensorProduct(
        lp.randprocs.covfuncs.Matern((), nu=2.5), lp.randprocs.covfuncs.Matern((), nu=2.5)))
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        prior.condition_on_observations(np.zeros(2), L=A @ V.to_linfunctl(X))
    monkeypatch.setattr(config, "matrix_free", True)
    with pytest.raises(NotImplementedError, match="A @ L.*matrix-free"):
        prior.condition_on_observations(np.zeros(2), L=A @ ev)
    monkeypatch.setattr(config, "matrix_free", False)
    monkeypatch.setattr(_spawn, "_active", object())
    with pytest.raises(NotImplementedError, match="A @ L.*lp.spawn"):
        prior.condition_on_observations(np.zeros(2), L=A @ ev)


def test_stencil_table_header_under_sanitizers(tmp_path):
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "mix_check")
    # the sanitizer runtimes are linked INTO the program, so that it does not care what else the environment loads before it
    clang = "clang" in subprocess.run([gxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static_rt, "-Wall", "-Wextra", "-I" + CSRC, os.path.join(CSRC, "hosttest", "mix_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + "\n" + res.stderr[-4000:]
    assert "mix_check: all checks passed" in res.stdout
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr
