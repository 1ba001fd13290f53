"""`diffops.VariableCoefficientOperator` on the host: the algebra of the class, its introspection, `L(m)` against closed
forms, shape and type errors, and the refusals that are decided without a device."""
import numpy as np
import pytest

import linpde_gp_amd as lp
from linpde_gp_amd import functions as fn
from linpde_gp_amd.linfuncops import Identity, diffops
from linpde_gp_amd.linfuncops.diffops import VariableCoefficientOperator as VCO

cf = lp.randprocs.covfuncs


def _lam(f, shape=()):
    return fn.LambdaFunction(f, shape)


def test_terms_merge_by_coefficient_object_and_keep_their_order():
    a, c = fn.Polynomial([1.0, 0.5]), _lam(np.sin)
    L = VCO((), [(a, -1.0 * diffops.Derivative(2)), (c, diffops.Derivative(0)), (a, 3.0 * diffops.Derivative(1)), (None, diffops.Derivative(1)),
                 (None, 2.0 * diffops.Derivative(1))])
    assert [f for f, _ in L.terms] == [a, c, None] and L.coefficient_functions == (a, c, None)
    assert L.terms[0][1] == {(2,): -1.0, (1,): 3.0}
    assert L.terms[1][1] == {(0,): 1.0}
    assert L.terms[2][1] == {(1,): 3.0}
    # an equal but distinct function object is its own term
    L2 = VCO((), [(fn.Polynomial([1.0]), diffops.Derivative(1)), (fn.Polynomial([1.0]), diffops.Derivative(1))])
    assert len(L2.terms) == 2
    # the returned maps are copies
    L.terms[0][1][(2,)] = 99.0
    assert L.terms[0][1][(2,)] == -1.0


def test_scaling_negation_and_flattening_sums():
    a, v = _lam(lambda x: 1.0 + x[..., 0], (2,)), _lam(lambda x: x[..., 1], (2,))
    lap, dx = diffops.Laplacian((2,)), diffops.DirectionalDerivative([1.0, 0.0])
    L = VCO((2,), [(a, lap), (v, dx)])
    assert (-L).terms[0][1] == {(2, 0): -1.0, (0, 2): -1.0} and (-L).terms[1][1] == {(1, 0): -1.0}
    assert (2.5 * L).terms[1][1] == {(1, 0): 2.5} and [f for f, _ in (2.5 * L).terms] == [a, v]
    S = L + 2.0 * Identity((2,))                  # a constant-coefficient operator joins as the term of the constant 1
    assert isinstance(S, VCO) and [f for f, _ in S.terms] == [a, v, None] and S.terms[2][1] == {(0, 0): 2.0}
    S2 = dx + L                                   # ... from the left as well
    assert isinstance(S2, VCO) and [f for f, _ in S2.terms] == [None, a, v] and S2.terms[0][1] == {(1, 0): 1.0}
    M = VCO((2,), [(v, lap), (None, dx)])
    T = L - M                                     # two variable operators: one flat list, shared functions merged
    assert isinstance(T, VCO) and [f for f, _ in T.terms] == [a, v, None]
    assert T.terms[1][1] == {(1, 0): 1.0, (2, 0): -1.0, (0, 2): -1.0} and T.terms[2][1] == {(1, 0): -1.0}
    D = lap - L
    assert isinstance(D, VCO) and D.terms[0] == (None, {(2, 0): 1.0, (0, 2): 1.0}) and D.terms[1][1] == {(2, 0): -1.0, (0, 2): -1.0}
    with pytest.raises(TypeError):
        L + 1.0
    with pytest.raises(TypeError):
        [1.0, 2.0] * L


def test_the_cap_on_the_number_of_terms_names_itself():
    fs = [_lam(np.sin) for _ in range(5)]
    VCO((), [(f, diffops.Derivative(1)) for f in fs[:4]])
    with pytest.raises(NotImplementedError, match="at most 4"):
        VCO((), [(f, diffops.Derivative(1)) for f in fs])
    L4 = VCO((), [(f, diffops.Derivative(1)) for f in fs[:4]])
    with pytest.raises(NotImplementedError, match="LPGP_MAXW"):
        L4 + diffops.Derivative(2)                # the constant term would be the fifth
    assert len((L4 + VCO((), [(fs[0], diffops.Derivative(2))])).terms) == 4


def test_shape_and_type_errors():
    a1, a2 = _lam(np.sin), _lam(lambda x: x[..., 0], (2,))
    with pytest.raises(ValueError):
        VCO((), [])
    with pytest.raises(TypeError):
        VCO((), [(np.sin, diffops.Derivative(1))])                        # a bare callable is not a Function
    with pytest.raises(TypeError):
        VCO((), [(a1, "d/dx")])
    with pytest.raises(TypeError):
        VCO((), [a1])
    with pytest.raises(ValueError):
        VCO((2,), [(a1, diffops.Laplacian((2,)))])                        # coefficient of the wrong input shape
    with pytest.raises(ValueError):
        VCO((), [(a1, diffops.Laplacian((2,)))])                          # operator of the wrong input shape
    with pytest.raises(ValueError):
        VCO((2,), [(fn.Constant((2,), np.ones(3)), diffops.Laplacian((2,)))])      # vector-valued coefficient
    with pytest.raises(TypeError):
        VCO((), [(a1, VCO((), [(a1, diffops.Derivative(1))]))])           # nesting: add them instead
    with pytest.raises(ValueError):
        VCO((2, 2), [(None, diffops.Laplacian((2,)))])
    L = VCO((2,), [(a2, diffops.Laplacian((2,)))])
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        L.coefficients_dict()
    with pytest.raises(ValueError):
        L(fn.Polynomial([1.0, 2.0]))                                      # a function of the real line
    W = L.weights(np.arange(12.0).reshape(2, 3, 2))
    assert W.shape == (1, 6) and np.array_equal(W[0], np.arange(0.0, 12.0, 2.0))


def test_applied_to_polynomial_affine_and_lambda_means():
    x = np.linspace(-1.0, 1.0, 17)
    # L = -a d^2 - a' d, a = 1 + x/2: the divergence form -(a u')'
    a, da = fn.Polynomial([1.0, 0.5]), fn.Polynomial([0.5])
    L = VCO((), [(a, -1.0 * diffops.Derivative(2)), (da, -1.0 * diffops.Derivative(1))])
    m = fn.Polynomial([2.0, -1.0, 0.5, 3.0])                             # m' = -1 + x + 9 x^2, m'' = 1 + 18 x
    np.testing.assert_allclose(L(m)(x), -(1 + x / 2) * (1 + 18 * x) - 0.5 * (-1 + x + 9 * x**2), rtol=0, atol=1e-14)
    # a constant term (f = None) and a reaction term on a scalar affine mean
    L2 = L + VCO((), [(_lam(np.cos), diffops.Derivative(0))]) + 2.0 * diffops.Derivative(1)
    m2 = fn.Affine(3.0, -1.0)
    np.testing.assert_allclose(L2(m2)(x), -0.5 * 3.0 + np.cos(x) * (3 * x - 1) + 6.0, rtol=0, atol=1e-14)
    # 2-D: -(1 + 0.3 x y) Lap + (y, -x) . grad + 2 on m = sin(x) cos(2 y) with supplied derivatives
    X = np.random.default_rng(0).uniform(-1, 1, (5, 7, 2))
    sx, cx, s2y, c2y = (lambda z: np.sin(z[..., 0])), (lambda z: np.cos(z[..., 0])), (lambda z: np.sin(2 * z[..., 1])), (lambda z: np.cos(2 * z[..., 1]))
    m3 = fn.LambdaFunction(lambda z: sx(z) * c2y(z), (2,), derivatives={
        (1, 0): lambda z: cx(z) * c2y(z), (0, 1): lambda z: -2 * sx(z) * s2y(z),
        (2, 0): lambda z: -sx(z) * c2y(z), (0, 2): lambda z: -4 * sx(z) * c2y(z)})
    L3 = VCO((2,), [(_lam(lambda z: 1 + 0.3 * z[..., 0] * z[..., 1], (2,)), -1.0 * diffops.Laplacian((2,))),
                    (_lam(lambda z: z[..., 1], (2,)), diffops.DirectionalDerivative([1.0, 0.0])),
                    (_lam(lambda z: -z[..., 0], (2,)), diffops.DirectionalDerivative([0.0, 1.0])),
                    (None, 2.0 * Identity((2,)))])
    xx, yy = X[..., 0], X[..., 1]
    ref = (1 + 0.3 * xx * yy) * 5 * np.sin(xx) * np.cos(2 * yy) + yy * np.cos(xx) * np.cos(2 * yy) + xx * 2 * np.sin(xx) * np.sin(2 * yy) \
        + 2 * np.sin(xx) * np.cos(2 * yy)
    out = L3(m3)(X)
    assert out.shape == (5, 7)
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-14)
    # a constant mean: only the order-0 parts survive; a missing derivative raises as for constant-coefficient operators
    np.testing.assert_allclose(L3(fn.Constant((2,), 1.5))(X), np.full((5, 7), 3.0))
    with pytest.raises(NotImplementedError):
        L3(fn.LambdaFunction(lambda z: z[..., 0], (2,)))(X)


def test_the_functional_carries_weights_and_term_maps():
    X = np.linspace(0.0, 1.0, 9)
    a = fn.Polynomial([1.0, 0.5])
    L = VCO((), [(a, -1.0 * diffops.Derivative(2)), (None, diffops.Derivative(0))])
    F = L.to_linfunctl(X)
    W, terms = F.variable_terms()
    assert W.shape == (2, 9) and np.array_equal(W[0], 1.0 + 0.5 * X) and np.array_equal(W[1], np.ones(9))
    assert terms == [{(2,): -1.0}, {(0,): 1.0}]
    W2, _ = (-2.0 * F).variable_terms()
    assert np.array_equal(W2, -2.0 * W)
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        F.coefficients_dict()
    with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
        (F + F).variable_terms()
    m = fn.Polynomial([0.0, 0.0, 1.0])
    np.testing.assert_allclose(F(m), -(1 + 0.5 * X) * 2 + X**2, rtol=0, atol=1e-15)
    # a constant-coefficient functional has none
    assert diffops.Derivative(1).to_linfunctl(X).variable_terms() is None


def test_read_outs_are_refused_before_any_device_work():
    k = cf.Matern((), nu=2.5)
    prior = lp.GaussianProcess(fn.Zero(()), k)
    L = VCO((), [(fn.Polynomial([1.0, 0.5]), diffops.Derivative(1))])
    for target in (k, prior):
        with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
            L(target)
        with pytest.raises(NotImplementedError, match="VariableCoefficientOperator"):
            L.to_linfunctl(np.linspace(0, 1, 4))(target)


def test_matrix_free_and_spawn_fronts_refuse(monkeypatch):
    from linpde_gp_amd import _spawn, config
    prior = lp.GaussianProcess(fn.Zero(()), cf.Matern((), nu=2.5))
    L = VCO((), [(fn.Polynomial([1.0, 0.5]), diffops.Derivative(1))])
    X, Y = np.linspace(0, 1, 5), np.zeros(5)
    monkeypatch.setattr(config, "matrix_free", True)
    with pytest.raises(NotImplementedError, match="matrix-free"):
        prior.condition_on_observations(Y, X, L=L)
    monkeypatch.setattr(config, "matrix_free", False)
    monkeypatch.setattr(_spawn, "_active", object())
    with pytest.raises(NotImplementedError, match="lp.spawn"):
        prior.condition_on_observations(Y, X, L=L)
    with pytest.raises(NotImplementedError, match="lp.spawn"):
        prior.condition_on_observations(Y, L=L.to_linfunctl(X))


@pytest.mark.parametrize("name", ["1d boundary first", "1d pde first", "2d grid", "two variable blocks"])
def test_the_dense_references_of_the_gpu_tests_are_well_conditioned(name):
    """The problems of tests/test_gpu_varcoef.py are compared with SciPy's Cholesky posterior at 1e-8 relative: SciPy itself must sit
    well inside that bar.  Against the long-double refinement of `oracle/gp.py` it is at most 5e-10 away (the variance of the 1-D
    problem, which is 1e-6 of the prior's) and 6e-11 on the representer weights; condition numbers 3e6, 1.5e9 and 6e7.  Asserted
    here with a tenth of the bar."""
    import _varcoef_reference as vr
    if name.startswith("1d"):
        kernel, obs, Xt = vr.problem_1d(name[3:])
    elif name == "2d grid":
        kernel, obs, Xt = vr.problem_2d()[:3]
    else:
        kernel, obs, Xt = vr.problem_two_variable_blocks()
    R = vr.Reference(kernel, obs)
    mean, var = R.predict(Xt)
    rm, rv, rw = R.refined(Xt)
    for got, want in ((mean, rm), (var, rv), (R.w, rw)):
        assert np.max(np.abs(got - want)) <= 1e-9 * np.max(np.abs(want))
