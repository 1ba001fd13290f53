"""Wendland compact-support priors (`LPGP_WENDLAND`, `LPGP_WENDLAND_ISO`) on the device: the reference's own suite
(`tests/linpde_gp/randprocs/cov/test_wendland.py`: matrix and linop), derivative blocks entry by entry against exact rational
blocks, the edge of the support and the tiles that are skipped, the Kronecker path, and a posterior through the public interface.

Bounds.  Gram entries: 4e-15 of the block maximum (the standing standard of test_gpu_parity.py), exactly 0.0 wherever the exact
scaled distance exceeds 1.  Derivative entries: |got - exact| <= K_DEVICE eps E, E the envelope of `_wendland_reference.py`,
K_DEVICE = 4 x the worst ratio of the NumPy fp64 helper measured on the CPU (10.90 -> 43.6).  Posterior: `posterior_tolerances`
(1e-8) against fp64 LAPACK, whose own error on this problem is asserted <= 1e-10 in tests/test_wendland_host.py."""
import numpy as np
import pytest

import _wendland_reference as ref
from conftest import posterior_tolerances

pytestmark = pytest.mark.gpu
EPS = 2.0**-53
GRAM_RTOL = 4e-15


@pytest.fixture(scope="module")
def lp():
    import linpde_gp_amd
    return linpde_gp_amd


@pytest.fixture(scope="module")
def ctx(lp):
    from linpde_gp_amd import _engine
    return _engine.default_context()


def _covfunc(lp, kernel):
    """The public covariance function of a reference kernel spec."""
    cf = lp.randprocs.covfuncs
    out = None
    for scale, spec in kernel:
        if spec[0] == "prod":
            fs = [cf.WendlandCovarianceFunction((), k=kp, lengthscales=ls) if f == "w" else cf.Matern((), nu=kp + 0.5, lengthscales=ls)
                  for f, kp, ls in spec[1]]
            k = cf.TensorProduct(*fs) if len(fs) > 1 else fs[0]
        else:
            k = cf.WendlandCovarianceFunction((len(spec[2]),), k=spec[1], lengthscales=spec[2])
        k = k if scale == 1.0 else scale * k
        out = k if out is None else out + k
    return out


def _hold_gram(what, got, G, OUT):
    err = float(np.abs(got - G).max() / np.abs(G).max())
    print(f"{what}: max |err| = {err:.2e} of the block maximum (bound {GRAM_RTOL:.0e}); {OUT.mean():.0%} of the entries outside the support")
    assert np.isfinite(got).all(), what
    assert (got[OUT] == 0.0).all(), what
    assert err <= GRAM_RTOL, (what, err)


def _hold_entries(what, got, G, E, OUT):
    err = np.abs(got - G)
    m = E > 0
    ratio = float(np.max(err[m] / (EPS * E[m]))) if m.any() else 0.0
    print(f"{what}: worst |err| / (eps E) = {ratio:.2f} (K = {ref.K_DEVICE:.1f}); {OUT.mean():.0%} outside the support")
    assert np.isfinite(got).all(), what
    assert (got[OUT] == 0.0).all(), what
    assert (err <= ref.K_DEVICE * EPS * E).all(), (what, ratio)


# ---- the reference's suite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,k", [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2), (4, 3), (1, 3), (2, 3)])
def test_matrix_and_linop_of_the_reference_suite(lp, d, k):
    """`cov.matrix(x0)` for 100 points of [-1, 1]^d against the exact values; `cov.linop(x0) @ eye` against `matrix` at the
    reference's atol = 1e-12."""
    cf = lp.randprocs.covfuncs
    x0 = np.random.default_rng(413 + 10 * d + k).uniform(-1.0, 1.0, (100, d))
    cov = cf.WendlandCovarianceFunction((d,), k)
    assert (cov.d, cov.k) == (d, k)
    kern = [(1.0, ("prod", [("w", k, 1.0)]))] if d == 1 else [(1.0, ("iso", k, [1.0] * d))]
    G, _, OUT = ref.exact_block(kern, ref.identity(d), ref.identity(d), x0, x0)
    K = cov.matrix(x0)
    _hold_gram(f"matrix d={d} k={k}", K, G, OUT)
    assert (np.diag(K) == 1.0).all()
    np.testing.assert_allclose(cov.linop(x0) @ np.eye(100), K, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov(x0[:7], x0[:7]), np.diag(K)[:7], rtol=0, atol=0)


def test_lengthscales_per_dimension(lp):
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(9)
    x0, x1 = rng.uniform(-1, 1, (70, 3)), rng.uniform(-1, 1, (45, 3))
    ls = [0.9, 0.5, 1.4]
    G, _, OUT = ref.exact_block([(1.0, ("iso", 2, ls))], ref.identity(3), ref.identity(3), x0, x1)
    _hold_gram("d=3 k=2, three lengthscales", cf.WendlandCovarianceFunction((3,), 2, lengthscales=ls).matrix(x0, x1), G, OUT)


# ---- derivative blocks -------------------------------------------------------------------------------------------------------
_CASES = ref.derivative_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_derivative_blocks_entry_by_entry(lp, ctx, case):
    """Ragged 150 x 70 (three by two tiles, partial last tiles): the dense block and the matrix-free product with the identity."""
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    name, kern, L0, L1 = case
    d = len(next(iter(L0)))
    rng = np.random.default_rng(sum(map(ord, name)))
    X0, X1 = ref.dyadic_points(rng, 150, d, bits=5 if d > 1 else 7), ref.dyadic_points(rng, 70, d, bits=5 if d > 1 else 7)
    G, E, OUT = ref.exact_block(kern, L0, L1, X0, X1)
    desc = cf.lower_groups(ref.base_groups(kern), L0, L1)
    assert desc == cf.DifferentiatedCovarianceFunction(_covfunc(lp, kern), L0, L1).lower()       # the public objects lower to the same groups
    P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
    _hold_entries(f"{name} block", _engine.kernel_matrix(ctx, desc, P0, P1), G, E, OUT)
    _hold_entries(f"{name} matvec", _engine.kernel_matvec(ctx, desc, P0, P1, np.eye(70)), G, E, OUT)


def test_variable_coefficient_block_on_a_tensor_product_prior(lp, ctx):
    """Two pairs with weights that are signed powers of two (exact products): the bound carries over with E = sum_p |w0 w1| E_p."""
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    kern = [(1.3, ("prod", [("w", 2, 0.7), ("w", 3, 0.9)]))]
    mlap, ident, dx = {(2, 0): -1.0, (0, 2): -1.0}, ref.identity(2), {(1, 0): 1.0, (0, 0): 0.5}
    rng = np.random.default_rng(21)
    X0, X1 = ref.dyadic_points(rng, 150, 2, bits=5), ref.dyadic_points(rng, 70, 2, bits=5)
    P0, P1 = _engine.Points(ctx, X0), _engine.Points(ctx, X1)
    pairs = [(mlap, mlap), (dx, ident)]
    descs = [cf.lower_groups(ref.base_groups(kern), a, b) for a, b in pairs]
    w0 = np.stack([2.0 ** rng.integers(-2, 3, 150) * rng.choice([-1.0, 1.0], 150) for _ in range(2)])
    w1 = np.stack([2.0 ** rng.integers(-2, 3, 70) * rng.choice([-1.0, 1.0], 70) for _ in range(2)])
    M = _engine.GramMatrix(ctx)
    M.add_block(70)
    M.add_block(150)
    M.assemble(descs[0], P1, None, 0, 0)
    M.assemble_weighted([(descs[0], 0, 0), (descs[1], 1, 1)], w0, w1, P0, P1, 1, 0)
    got = M.todense("gram")[70:, :70]
    want, env, out = np.zeros((150, 70)), np.zeros((150, 70)), None
    for q, (a, b) in enumerate(pairs):
        G, E, OUT = ref.exact_block(kern, a, b, X0, X1)
        W = np.outer(w0[q], w1[q])
        want, env, out = want + W * G, env + np.abs(W) * E, OUT
    _hold_entries("weighted, two pairs", got, want, env, out)


# ---- the edge of the support and empty tiles ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    """x_i = i / 64, i = 0 .. 299, l = 0.5, k = 2: everything exactly representable; pairs with r == 1 exactly (|i - j| = 32), tiles
    wholly out of reach (|i - j| > 32 throughout), straddling tiles, and a last tile of 44 rows."""
    x = np.arange(300) / 64.0
    kern = [(1.0, ("prod", [("w", 2, 0.5)]))]
    G, E, OUT = ref.exact_block(kern, ref.identity(1), ref.identity(1), x, x)
    i = np.arange(300)
    assert (OUT == (np.abs(i[:, None] - i[None, :]) > 32)).all() and G[0, 32] == 0.0 and not OUT[0, 32] and G[0, 31] > 0.0
    return x, kern, G, OUT


def test_edge_of_the_support_and_empty_tiles_1d(lp, ctx, edge):
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    x, kern, G, OUT = edge
    cov = cf.WendlandCovarianceFunction((), k=2, lengthscales=0.5)
    desc = cov.lower()
    P = _engine.Points(ctx, x[:, None])
    _hold_gram("edge: rectangular block", cov.matrix(x), G, OUT)
    _hold_gram("edge: rectangular block, 300 x 130", cov.matrix(x, x[170:]), G[:, 170:], OUT[:, 170:])
    M = _engine.GramMatrix(ctx)
    M.add_block(300)
    M.assemble(desc, P, None, 0, 0)
    _hold_gram("edge: lower-only Gram", M.todense("gram"), G, OUT)
    perm = np.random.default_rng(3).permutation(300)
    _hold_gram("edge: shuffled", cov.matrix(x[perm]), G[np.ix_(perm, perm)], OUT[np.ix_(perm, perm)])
    # sorted and shuffled give the same bits entry by entry: the skipped tiles hold what the evaluation would have written
    assert np.array_equal(cov.matrix(x[perm])[np.ix_(np.argsort(perm), np.argsort(perm))], cov.matrix(x))
    # first derivatives: a class that flips signs, zeros of either sign must still compare equal to 0.0
    d1 = {(1,): 1.0}
    G1, E1, OUT1 = ref.exact_block(kern, d1, d1, x, x[170:])
    _hold_entries("edge: d/dx d/dx'", _engine.kernel_matrix(ctx, cf.lower_groups(ref.base_groups(kern), d1, d1), P, _engine.Points(ctx, x[170:, None])),
                  G1, E1, OUT1)


def test_sorted_isotropic_set_and_the_matrix_free_product(lp, ctx):
    """300 x 200 points in 2-D sorted by their first coordinate, d = 2, k = 2, l = 0.25: tiles out of reach along the first axis.
    The product K V against the exact dense block times V: an entry inside the support is good to GRAM_RTOL (of the block maximum,
    1), one outside is exactly 0; the sum of a row has depth <= 200 (one fma per column, then waves and splits in a fixed order) --
    |err_i| <= GRAM_RTOL sum_{j inside} |V_j| + 200 eps sum_j |K_ij| |V_j|, as test_gpu_pcg_kernels.py derives its bounds from the depth
    of the sum."""
    from linpde_gp_amd import _engine
    cf = lp.randprocs.covfuncs
    rng = np.random.default_rng(17)
    X0 = np.column_stack([np.sort(rng.uniform(-1, 1, 300)), rng.uniform(-1, 1, 300)])
    X1 = np.column_stack([np.sort(rng.uniform(-1, 1, 200)), rng.uniform(-1, 1, 200)])
    ls = [0.25, 0.5]
    cov = cf.WendlandCovarianceFunction((2,), 2, lengthscales=ls)
    G, _, OUT = ref.exact_block([(1.0, ("iso", 2, ls))], ref.identity(2), ref.identity(2), X0, X1)
    K = cov.matrix(X0, X1)
    _hold_gram("sorted isotropic 300 x 200", K, G, OUT)
    tiles_out = sum(OUT[i:i + 64, j:j + 64].all() for i in range(0, 300, 64) for j in range(0, 200, 64))
    print(f"{tiles_out} of 20 tiles wholly outside the support")
    assert tiles_out >= 4
    perm0, perm1 = rng.permutation(300), rng.permutation(200)
    assert np.array_equal(cov.matrix(X0[perm0], X1[perm1]), K[np.ix_(perm0, perm1)])
    V = rng.standard_normal((200, 5))
    got = cov.linop(X0, X1) @ V
    want = (G.astype(np.longdouble) @ V.astype(np.longdouble)).astype(np.double)
    bound = GRAM_RTOL * ((~OUT).astype(np.double) @ np.abs(V)) + 200 * EPS * (np.abs(G) @ np.abs(V))
    err = np.abs(got - want)
    print(f"matrix-free product: worst err / bound = {np.max(err[bound > 0] / bound[bound > 0]):.3f}")
    assert (err <= bound).all()
    assert np.array_equal((cov.linop(X0[perm0], X1) @ V), got[perm0])      # rows are independent of their tile's neighbours


def test_tensor_grid_gram_kronecker_and_entry_wise(lp, ctx, kronecker_everywhere):
    from linpde_gp_amd import _engine, config, domains
    cf = lp.randprocs.covfuncs
    g0, g1 = np.linspace(-1.0, 1.0, 16), np.linspace(-0.5, 1.0, 16)
    kern = [(1.0, ("prod", [("w", 2, 0.7), ("w", 1, 0.6)]))]
    cov = _covfunc(lp, kern)
    grid = domains.TensorProductGrid(g0, g1)
    X = np.asarray(grid).reshape(-1, 2)
    G, _, OUT = ref.exact_block(kern, ref.identity(2), ref.identity(2), X, X)
    saved = config.use_grid_assembly
    try:
        for path in ("kron", "entry"):
            config.use_grid_assembly = path == "kron"
            P = _engine.as_points(ctx, grid, X)
            assert (P.grid_factors is not None) == (path == "kron")
            M = _engine.GramMatrix(ctx)
            M.add_block(256)
            ctx.profile_reset()
            ctx.profile_enable(["assemble_grid"])
            M.assemble(cov.lower(), P, None, 0, 0)
            got = M.todense("gram")
            launches = ctx.profile_get()["assemble_grid"]["launches"]
            ctx.profile_enable(False)
            assert (launches >= 1) == (path == "kron")
            _hold_gram(f"16 x 16 grid, {path}", got, G, OUT)
    finally:
        config.use_grid_assembly = saved
        ctx.profile_enable(False)


# ---- posterior ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["lazy", "eager"])
def factorization_check(lp, request):
    saved = lp.config.lazy_factorization
    lp.config.lazy_factorization = request.param == "lazy"
    yield request.param
    lp.config.lazy_factorization = saved


def _prior(lp):
    return lp.GaussianProcess(lp.functions.Zero((2,)), _covfunc(lp, ref.POST_KERNEL))


@pytest.fixture(scope="module")
def lapack():
    return ref.posterior_lapack()


def test_posterior_against_lapack(lp, lapack, factorization_check):
    """10 x 10 interior collocation of -Lap (rhs 2), 4 x 12 boundary values under Normal(0, 1e-8 I), 64 prediction points.
    Algebraic parity only: with this support and spacing the posterior mean is far from the PDE's solution."""
    from linpde_gp_amd.linfuncops import diffops
    Xc, yc, Xb, yb, Xt = ref.posterior_problem()
    noise = lp.randvars.Normal(np.zeros(48), ref.POST_NUGGET * np.eye(48))
    u = _prior(lp).condition_on_observations(yc, X=Xc, L=-1.0 * diffops.Laplacian((2,)))
    u = u.condition_on_observations(yb, X=Xb, b=noise)
    mean, var = u.predict(Xt)
    ma, va = posterior_tolerances(lapack["mean"], lapack["var"])
    em, ev = np.abs(mean - lapack["mean"]).max(), np.abs(var - lapack["var"]).max()
    print(f"{factorization_check}: mean err {em:.3e} / {ma:.3e}   var err {ev:.3e} / {va:.3e}   cond {lapack['cond']:.2e}")
    assert em <= ma and ev <= va


def test_posterior_diagnostics_sampling_and_the_gradient_refusal(lp, lapack):
    from linpde_gp_amd.linfuncops import diffops
    Xc, yc, Xb, yb, Xt = ref.posterior_problem()
    noise = lp.randvars.Normal(np.zeros(48), ref.POST_NUGGET * np.eye(48))
    u1 = _prior(lp).condition_on_observations(yc, X=Xc, L=-1.0 * diffops.Laplacian((2,)))
    u = u1.condition_on_observations(yb, X=Xb, b=noise)
    mean, var = u.predict(Xt)
    # the boundary block appended as a second conditioning of a fresh chain gives the same posterior
    v = _prior(lp).condition_on_observations(yc, X=Xc, L=-1.0 * diffops.Laplacian((2,))).condition_on_observations(yb, X=Xb, b=noise)
    mean2, var2 = v.predict(Xt)
    assert np.abs(mean2 - mean).max() <= 1e-12 * np.abs(mean).max() and np.abs(var2 - var).max() <= 1e-12 * np.abs(var).max()
    # the parent still answers for its own block
    m1, v1 = u1.predict(Xt)
    assert np.isfinite(m1).all() and (v1 >= var - 1e-9).all()
    draws = u.sample(np.random.default_rng(0), Xt[:10], size=3)
    again = u.sample(np.random.default_rng(0), Xt[:10], size=3)
    assert draws.shape == (3, 10) and np.isfinite(draws).all() and np.array_equal(draws, again)
    lml = u.log_marginal_likelihood()
    loo = u.leave_one_out()
    print(f"lml {lml:.12e} (LAPACK {lapack['lml']:.12e}); loo mean err {np.abs(loo.mean - lapack['loo_mean']).max():.2e}, "
          f"var err {np.abs(loo.var - lapack['loo_var']).max():.2e}")
    assert abs(lml - lapack["lml"]) <= 1e-8 * abs(lapack["lml"])
    assert np.abs(loo.mean - lapack["loo_mean"]).max() <= 1e-8 * np.abs(lapack["loo_mean"]).max()
    assert np.abs(loo.var - lapack["loo_var"]).max() <= 1e-8 * np.abs(lapack["loo_var"]).max()
    cov = u.cov.linop(Xt[:9]).todense()
    np.testing.assert_allclose(np.diag(cov), var[:9], rtol=0, atol=1e-8 * np.abs(lapack["var"]).max())
    with pytest.raises(NotImplementedError, match="Wendland"):
        u.log_marginal_likelihood_gradient()
